#!/usr/bin/env python3
"""The collocation backend in a wind field at batch scale: B perturbed copies of the reference's exp_14 (121 nodes, hard bounds;
d2dhip.synth.nlp_problems) and one problem alone, in constant wind through d2d_nlp_solve and in a steady (shear) and an unsteady
(gust) field through d2d_nlp_solve_wind.  The fields are tests/wind_ref.py's with the planner's sign (-F: the plan of a plant that flies
F; the shear then blows along the leg, and every problem stays feasible below v_max).  HIP events, best of 3 after a warm-up.
python tools/bench_nlp_wind.py [B ...]     (default 4096 1)
python tools/bench_nlp_wind.py groups [R]  the multi-aircraft problem (d2d_nlp_solve_groups_wind): R (default 1024) perturbed copies of
    the trap_4-like scenarios of tests/nlp_groups_wind_ref.py (4 aircraft, 61 nodes, the collision pair active) in the steady shear
    and the unsteady gust, against d2d_nlp_solve_groups on the same scenarios in the constant wind of the field's mean; then the
    wall time of the three-formation mission of tests/test_gpu_mission_wind.py (one pass of phase 3) with and without its field.  Median of 5 timed
    launches after a warm-up, HIP events, one process.
python tools/bench_nlp_wind.py pairs [R]   collision avoidance on every pair (d2d_nlp_solve_groups_pairs): R (default 1024) perturbed copies
    of four-aircraft scenarios in constant wind, (i) the default pair through d2d_nlp_solve_groups, three repeats of the whole
    measurement (their spread is the noise band), (ii) the same rows with the masks of the pair (0, 1) through the new entry point,
    (iii) all six pairs; on the side-by-side layouts of tests/nlp_groups_wind_ref.py and on the crossing layouts of
    tests/nlp_groups_pairs_ref.py.  Median of 5 timed launches after a warm-up, HIP events, one process.
python tools/bench_nlp_wind.py moving [B]  moving obstacles (d2d_nlp_solve_moving): B (default 4096) perturbed exp_14 at 121 nodes with 0,
    1 and 4 moving discs against the SAME problems with the same number of static discs in the row through d2d_nlp_solve -- the
    tracks stand still where the static discs are, so both entries solve the same problems and the ratio is the cost of the centre
    planes and the rolled loop, not of the terms.  The two entries alternate, 1 warm-up + 5 timed launches each, HIP events, one
    process; medians and the spread of each.
python tools/bench_nlp_wind.py via [B]     timed waypoints (d2d_nlp_solve_via): B (default 4096) perturbed exp_14 at 121 nodes, each with one
    (x, y) pin at node 60 on the middle of its leg moved 5 m sideways, from the piecewise-linear guess through the pin, against the
    tool's own unpinned constant-wind figure (d2d_nlp_solve, the same rows from their own guess) in the same run.  The two entries
    alternate, 1 warm-up + 5 timed launches each, HIP events, one process; medians and the spread of each.
python tools/bench_nlp_wind.py free [B]    a free time step (d2d_nlp_solve_free): B (default 4096) perturbed exp_14 at 121 nodes, once with
    the step fixed (d2d_nlp_solve) and once with h free in [h / 2, 2 h] (k_dur = 0: the duration is whatever lets v sit at VSP), the
    same rows from the same guess.  The two entries alternate, 1 warm-up + 5 timed launches each, HIP events, one process; medians,
    the spread of each, the share CONVERGED of both and what the freed step does to the problems the fixed one leaves STALLED.
python tools/bench_nlp_wind.py keepout [B] hard keep-out discs (d2d_nlp_solve_keepout): B (default 4096) perturbed exp_14 at 121 nodes, each
    with one disc of 15 m whose centre lies on the middle of its leg moved 3 m sideways (node radius: KeepOut.lowered with the row's
    VMAX and h, no margin), against the same rows without a disc through d2d_nlp_solve, from the same guess.  The two entries
    alternate, 1 warm-up + 5 timed launches each, HIP events, one process; medians, the spread of each, statuses, mean and longest
    step counts, and the smallest g / R^2 of the converged plans.
python tools/bench_nlp_wind.py keepout-free [B] hard keep-out discs with the step free (d2d_nlp_solve_free_fence): the rows, the disc and the
    guess of `keepout`, once through d2d_nlp_solve_keepout at the fixed step h and twice through d2d_nlp_solve_free_fence with h free in
    [h / 2, 2 h], k_dur = 0 and no edges -- with the fixed solve's disc table (only the step changes) and with the table lowered for the
    largest step 2 h, as the planners lower it.  The three alternate, 1 warm-up + 5 timed launches each, HIP events, one process;
    medians and the spread of each, statuses, mean and longest step counts, what the freed step does to the problems the fixed one
    leaves STALLED, the solved durations and the smallest g / R^2 of the converged plans.
python tools/bench_nlp_wind.py keepout-moving [B] hard keep-out discs that move (d2d_nlp_solve_keepout_moving): the rows, the disc and the
    guess of `keepout`, the disc once held still through d2d_nlp_solve_keepout, once as a track that stands still and once crossing
    the leg at 3 m/s (at the static centre at mid-time; node radius MovingKeepOut.lowered) through d2d_nlp_solve_keepout_moving.  The
    three alternate, 1 warm-up + 5 timed launches each, HIP events, one process; medians, the spread of each, statuses, mean and
    longest step counts, the smallest g / R^2 of the converged plans, and whether the still track gives the static entry's bytes.
python tools/bench_nlp_wind.py fence [B]   a hard geofence (d2d_nlp_solve_fence): the rows, the disc and the guess of `keepout`, once through
    d2d_nlp_solve_keepout with the disc, once through d2d_nlp_solve_fence WITHOUT the disc inside a corridor round the leg (a
    d2d.opty_utils.GeoFence per problem: the side towards which the problem's free plan -- an untimed d2d_nlp_solve first -- leaves its
    leg's axis most lies at 0.8 of that excursion, the other three sides stand far off; beside the disc no edge can bind, a plan
    touches the disc in one point and the start rule needs kap of room there) and once through d2d_nlp_solve_fence with the disc and
    four ABSENT edges -- the price of the code path.  The three alternate, 1 warm-up + 5 timed launches each, HIP
    events, one process; medians, the spread of each, statuses, mean and longest step counts, the smallest g of the converged plans at
    the edges, and whether the absent edges give d2d_nlp_solve_keepout's bytes.
python tools/bench_nlp_wind.py guess [B]   the start of the solve (d2d_nlp_guess_dubins): B (default 4096) perturbed exp_14 at 121 nodes through
    d2d_nlp_solve from the host dog-leg (d2d.opty_utils.triangle, copied to the device) and from the Dubins start built on the device
    from the same rows.  The two starts alternate, 1 warm-up + 5 timed launches each, HIP events, one process; medians and the spread
    of each solve, the guess kernel's own time (at B and at 65 536 problems) beside the host's time for the dog-leg and its copy,
    statuses, mean and longest step counts, and the costs of the problems both starts converge on."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, _p)
import numpy as np


def groups_leg(R):
    import torch, d2dhip
    import d2dhip as D
    import nlp_groups_wind_ref as G
    import nlp_wind_ref as NR
    ctx = d2dhip.Context(0)
    rng = np.random.default_rng(7)
    base = G.group_scenarios()
    rows = np.concatenate([base[r % 3].copy() for r in range(R)])
    shift = np.repeat(rng.uniform(-3.0, 3.0, (R, 2)), G.N_AC, 0)              # a scenario moves as a whole: the pair keeps its gap
    rows[:, [D.SC_X0, D.SC_X1]] += shift[:, :1]; rows[:, [D.SC_Y0, D.SC_Y1]] += shift[:, 1:]
    W0 = np.stack([w.T for w in G.guesses(rows)])
    fields = NR.fields()
    for name, t_hi in (('shear', 0.0), ('gust', 6.0)):
        F = fields[name]
        mean = F.cp.mean(axis=(0, 2, 3))
        rows_c = rows.copy(); rows_c[:, D.SC_WX], rows_c[:, D.SC_WY] = -mean[0], -mean[1]
        t = ctx.dev(rng.uniform(0.0, t_hi, R) if t_hi > 0 else np.zeros(R))
        res = {}
        for kind in ('constant', 'field'):
            dsc = ctx.dev(rows_c if kind == 'constant' else rows)
            times = []
            for rep in range(6):                             # the first launch is the warm-up
                W = ctx.dev(np.ascontiguousarray(W0))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                out = ctx.nlp_solve_groups(dsc, W, G.H, G.N_AC) if kind == 'constant' else ctx.nlp_solve_groups_wind(dsc, W, G.H, G.N_AC, F, t)
                e1.record(); torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3)
            med = float(np.median(times[1:]))
            st = out['status'].cpu().numpy(); it = out['iters'].cpu().numpy(); sw = out['sweeps'].cpu().numpy()
            res[kind] = med
            print(json.dumps({'leg': 'groups', 'R': R, 'n_ac': G.N_AC, 'nodes': G.N_NODES, 'field': name, 'wind': kind, 'seconds_median': med,
                              'seconds_min': min(times[1:]), 'seconds_max': max(times[1:]), 'scenarios_per_s': R / med,
                              'aircraft_problems_per_s': R * G.N_AC / med, 'vs_constant': med / res['constant'],
                              'converged_frac': float((st == 1).mean()), 'mean_newton_steps': float(it.mean()), 'max_newton_steps': int(it.max()),
                              'mean_sweeps': float(sw.mean()), 'max_sweeps': int(sw.max())}), flush=True)
    ctx.close()
    # the mission of tests/test_gpu_mission_wind.py (three formations, the plan, its tracking, ONE pass of phase 3), with and without its
    # field: wall clock around the chain, device synchronised
    import time
    import full_sim as fs
    import multi_opt_planner as mop
    n_ac, c, X1_f, X2_f, X0B, ref3 = G.mission_inputs()
    cB = np.stack([c, c, c])
    dctx = d2dhip.default_context()
    for name, F in (('none', None), ('mission_field', G.mission_field())):
        ph1 = fs.CircularFormationGVF_batch(cB, 60, 15, n_ac, X0f=np.stack([X1_f] * 3)[:, :, :3], X0=X0B, record=(), windfield=F)
        t_end = G.mission_t_end(ph1['stop_row'].cpu().numpy(), len(ph1['time']), 0.05, 6, ref3[0], 1)
        times = []
        for rep in range(6):
            dctx.sync(); t0 = time.perf_counter()
            out = fs.full_sim_phases_batch(cB, 60, 15, n_ac, X1_f, mop.trap_4, X2_f, 6, ref3=ref3, t_sim_end=t_end, X0=X0B, windfield=F)
            dctx.sync(); times.append(time.perf_counter() - t0)
        print(json.dumps({'leg': 'mission', 'formations': 3, 'field': name, 'phase3_passes': len(out['phase3']),
                          'seconds_median': float(np.median(times[1:])), 'seconds_min': min(times[1:]), 'seconds_max': max(times[1:])}), flush=True)


def pairs_leg(R):
    import torch, d2dhip
    import d2dhip as D
    import nlp_groups_wind_ref as G
    import nlp_groups_pairs_ref as P
    ctx = d2dhip.Context(0)
    rng = np.random.default_rng(7)
    shift = np.repeat(rng.uniform(-3.0, 3.0, (R, 2)), G.N_AC, 0)              # a scenario moves as a whole: the gaps stay

    def batch(base):
        rows = np.concatenate([base[r % len(base)].copy() for r in range(R)])
        rows[:, [D.SC_X0, D.SC_X1]] += shift[:, :1]; rows[:, [D.SC_Y0, D.SC_Y1]] += shift[:, 1:]
        return rows

    def timed(label, layout, rows, W0, pairs_entry, max_sweeps):
        dsc = ctx.dev(rows)
        times = []
        for rep in range(6):                                 # the first launch is the warm-up
            W = ctx.dev(np.ascontiguousarray(W0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            out = (ctx.nlp_solve_groups_pairs if pairs_entry else ctx.nlp_solve_groups)(dsc, W, G.H, G.N_AC, max_sweeps=max_sweeps)
            e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        med = float(np.median(times[1:]))
        st = out['status'].cpu().numpy(); it = out['iters'].cpu().numpy(); sw = out['sweeps'].cpu().numpy()
        print(json.dumps({'leg': 'pairs', 'what': label, 'layout': layout, 'R': R, 'n_ac': G.N_AC, 'nodes': G.N_NODES, 'max_sweeps': max_sweeps,
                          'seconds_median': med, 'seconds_min': min(times[1:]), 'seconds_max': max(times[1:]), 'scenarios_per_s': R / med,
                          'aircraft_problems_per_s': R * G.N_AC / med, 'converged_frac': float((st == 1).mean()),
                          'mean_newton_steps': float(it.mean()), 'mean_sweeps': float(sw.mean()), 'min_sweeps': int(sw.min()),
                          'max_sweeps_seen': int(sw.max())}), flush=True)
        return med

    wind = (3.0, 0.0)                                        # the planner's constant wind: 9 m/s over the ground at 12 m/s of airspeed
    for layout, p01, pall, ms in (('side_by_side', [r.copy() for r in G.group_scenarios()], None, 12),
                                  ('crossing', P.pair_scenarios([(0, 1)]), P.pair_scenarios('all'), P.MAX_SWEEPS)):
        for r in p01:
            r[:, D.SC_WX], r[:, D.SC_WY] = -wind[0], -wind[1]
            r[0, D.SC_PMASK], r[1, D.SC_PMASK] = 0b10, 0b01          # (d2d_nlp_solve_groups does not read the column)
        if pall is None:
            pall = [P.pair_rows([tuple(q[D.SC_X0:D.SC_X0 + 3]) for q in r], [tuple(q[D.SC_X1:D.SC_X1 + 3]) for q in r], P.all_pairs(G.N_AC)) for r in p01]
        for r in pall:
            r[:, D.SC_WX], r[:, D.SC_WY] = -wind[0], -wind[1]
        rows01, rows_all = batch(p01), batch(pall)
        W0 = np.stack([w.T for w in G.guesses(rows01)])
        base = [timed('(i) default pair, d2d_nlp_solve_groups, repeat %d' % k, layout, rows01, W0, False, ms) for k in range(3)]
        same = timed('(ii) the same rows, d2d_nlp_solve_groups_pairs', layout, rows01, W0, True, ms)
        allp = timed('(iii) all six pairs, d2d_nlp_solve_groups_pairs', layout, rows_all, W0, True, ms)
        print(json.dumps({'leg': 'pairs', 'layout': layout, 'noise_band_of_i': (max(base) - min(base)) / float(np.median(base)),
                          'ii_over_i': same / float(np.median(base)), 'iii_over_i': allp / float(np.median(base))}), flush=True)
    ctx.close()


def moving_leg(B):
    import torch, d2dhip
    import d2dhip as D
    from d2dhip import synth
    from d2d.opty_utils import MovingObstacle, lower_moving
    ctx = d2dhip.Context(0)
    rows0, W0, h = synth.nlp_problems(B)
    rows0[:, D.SC_KOBS] = 1.0
    mid = 0.5 * (rows0[:, [D.SC_X0, D.SC_Y0]] + rows0[:, [D.SC_X1, D.SC_Y1]])
    offs = np.array([(4.0, -3.0), (-18.0, 14.0), (22.0, 10.0), (-6.0, -24.0)])      # disc centres relative to the middle of the leg
    radius = 7.0
    for n_disc in (0, 1, 4):
        rows_s = rows0.copy()
        for i in range(n_disc):
            c = D.obs_col(i)
            rows_s[:, c:c + 2] = mid + offs[i]; rows_s[:, c + 2] = radius
        kn = dc = None
        if n_disc:
            tabs = [lower_moving([MovingObstacle((0.0, 12.0), (mid[b] + offs[i], mid[b] + offs[i]), radius) for i in range(n_disc)]) for b in range(B)]
            kn, dc = ctx.dev(np.stack([t[0] for t in tabs])), ctx.dev(np.stack([t[1] for t in tabs]))
        dsc_s, dsc_m, t0 = ctx.dev(rows_s), ctx.dev(rows0), ctx.dev(np.zeros(B))
        times = {'static': [], 'moving': []}
        outs = {}
        for rep in range(6):                                 # the first launch of each is the warm-up; the entries alternate
            for what in ('static', 'moving'):
                W = ctx.dev(np.ascontiguousarray(W0))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                outs[what] = ctx.nlp_solve(dsc_s, W, h) if what == 'static' else ctx.nlp_solve_moving(dsc_m, W, h, kn, dc, None, t0 if n_disc else None)
                e1.record(); torch.cuda.synchronize()
                times[what].append(e0.elapsed_time(e1) * 1e-3)
        med = {k: float(np.median(v[1:])) for k, v in times.items()}
        for what in ('static', 'moving'):
            st = outs[what]['status'].cpu().numpy(); it = outs[what]['iters'].cpu().numpy()
            print(json.dumps({'leg': 'moving', 'B': B, 'nodes': W0.shape[2], 'discs': n_disc, 'entry': what, 'seconds_median': med[what],
                              'seconds_min': min(times[what][1:]), 'seconds_max': max(times[what][1:]), 'problems_per_s': B / med[what],
                              'moving_over_static': med['moving'] / med['static'], 'converged_frac': float((st == 1).mean()),
                              'mean_newton_steps': float(it.mean())}), flush=True)
    ctx.close()


def via_leg(B):
    import torch, d2dhip
    import d2dhip as D
    from d2dhip import synth
    from d2d.opty_utils import Waypoint, lower_waypoints, via_guess
    ctx = d2dhip.Context(0)
    rows, W0, h = synth.nlp_problems(B)
    N, node = W0.shape[2], 60
    p0, p1 = rows[:, D.SC_X0:D.SC_X0 + 3], rows[:, D.SC_X1:D.SC_X1 + 3]
    d = p1[:, :2] - p0[:, :2]
    d /= np.hypot(d[:, 0], d[:, 1])[:, None]
    pin = p0[:, :2] + (p1[:, :2] - p0[:, :2]) * node / (N - 1) + 5.0 * np.stack([-d[:, 1], d[:, 0]], 1)
    wps = [[Waypoint(node * h, pin[b, 0], pin[b, 1])] for b in range(B)]
    via = ctx.dev(np.stack([lower_waypoints(w, 0.0, h, N) for w in wps]))
    Wv = np.stack([np.stack(via_guess(p0[b], p1[b], wps[b], 0.0, h, N, rows[b, D.SC_VSP])) for b in range(B)])
    dsc = ctx.dev(rows)
    times = {'unpinned': [], 'via': []}
    outs = {}
    for rep in range(6):                                     # the first launch of each is the warm-up; the entries alternate
        for what in ('unpinned', 'via'):
            W = ctx.dev(np.ascontiguousarray(W0 if what == 'unpinned' else Wv))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            outs[what] = ctx.nlp_solve(dsc, W, h) if what == 'unpinned' else ctx.nlp_solve_via(dsc, W, h, via)
            e1.record(); torch.cuda.synchronize()
            times[what].append(e0.elapsed_time(e1) * 1e-3)
    med = {k: float(np.median(v[1:])) for k, v in times.items()}
    for what in ('unpinned', 'via'):
        st = outs[what]['status'].cpu().numpy(); it = outs[what]['iters'].cpu().numpy()
        print(json.dumps({'leg': 'via', 'B': B, 'nodes': N, 'entry': what, 'seconds_median': med[what], 'seconds_min': min(times[what][1:]),
                          'seconds_max': max(times[what][1:]), 'problems_per_s': B / med[what], 'via_over_unpinned': med['via'] / med['unpinned'],
                          'converged_frac': float((st == 1).mean()), 'mean_newton_steps': float(it.mean()), 'max_newton_steps': int(it.max())}),
              flush=True)
    ctx.close()


def free_leg(B):
    import torch, d2dhip
    from d2dhip import synth
    ctx = d2dhip.Context(0)
    rows, W0, h = synth.nlp_problems(B)
    dsc = ctx.dev(rows)
    fr = ctx.dev(np.tile([0.5 * h, 2.0 * h, 0.0, 0.0], (B, 1)))
    times = {'fixed': [], 'free': []}
    outs = {}
    for rep in range(6):                                     # the first launch of each is the warm-up; the entries alternate
        for what in ('fixed', 'free'):
            W = ctx.dev(np.ascontiguousarray(W0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            outs[what] = ctx.nlp_solve(dsc, W, h) if what == 'fixed' else ctx.nlp_solve_free(dsc, W, h, fr)
            e1.record(); torch.cuda.synchronize()
            times[what].append(e0.elapsed_time(e1) * 1e-3)
    med = {k: float(np.median(v[1:])) for k, v in times.items()}
    st = {k: outs[k]['status'].cpu().numpy() for k in outs}
    for what in ('fixed', 'free'):
        it = outs[what]['iters'].cpu().numpy()
        rec = {'leg': 'free', 'B': B, 'nodes': W0.shape[2], 'entry': what, 'seconds_median': med[what], 'seconds_min': min(times[what][1:]),
               'seconds_max': max(times[what][1:]), 'problems_per_s': B / med[what], 'free_over_fixed': med['free'] / med['fixed'],
               'converged_frac': float((st[what] == 1).mean()), 'stalled_frac': float((st[what] == 4).mean()),
               'mean_newton_steps': float(it.mean()), 'max_newton_steps': int(it.max())}
        if what == 'free':
            hh = outs['free']['h'].cpu().numpy()
            ok = st['free'] == 1
            rec.update(fixed_not_converged=int((st['fixed'] != 1).sum()), of_those_free_converged=int((ok & (st['fixed'] != 1)).sum()),
                       fixed_converged_free_not=int((~ok & (st['fixed'] == 1)).sum()),
                       duration_min_mean_max=[float(v) * (W0.shape[2] - 1) for v in (hh[ok].min(), hh[ok].mean(), hh[ok].max())] if ok.any() else None)
        print(json.dumps(rec), flush=True)
    ctx.close()


def keepout_leg(B):
    import torch, d2dhip
    import d2dhip as D
    from d2dhip import synth
    from d2d.opty_utils import KeepOut
    ctx = d2dhip.Context(0)
    rows, W0, h = synth.nlp_problems(B)
    N = W0.shape[2]
    p0, p1 = rows[:, D.SC_X0:D.SC_X0 + 2], rows[:, D.SC_X1:D.SC_X1 + 2]
    d = p1 - p0
    d /= np.hypot(d[:, 0], d[:, 1])[:, None]
    c = 0.5 * (p0 + p1) + 3.0 * np.stack([-d[:, 1], d[:, 0]], 1)
    discs = np.array([[KeepOut(c[b], 15.0).lowered(rows[b, D.SC_VMAX], h)] for b in range(B)])
    dsc, dk = ctx.dev(rows), ctx.dev(discs)
    times = {'plain': [], 'keepout': []}
    outs, Ws = {}, {}
    for rep in range(6):                                     # the first launch of each is the warm-up; the entries alternate
        for what in ('plain', 'keepout'):
            W = ctx.dev(np.ascontiguousarray(W0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            outs[what] = ctx.nlp_solve(dsc, W, h) if what == 'plain' else ctx.nlp_solve_keepout(dsc, W, h, dk)
            e1.record(); torch.cuda.synchronize()
            times[what].append(e0.elapsed_time(e1) * 1e-3)
            Ws[what] = W
    med = {k: float(np.median(v[1:])) for k, v in times.items()}
    for what in ('plain', 'keepout'):
        st = outs[what]['status'].cpu().numpy(); it = outs[what]['iters'].cpu().numpy()
        Wh = Ws[what].cpu().numpy()
        g = ((Wh[:, 0, 1:-1] - discs[:, 0, 0:1]) ** 2 + (Wh[:, 1, 1:-1] - discs[:, 0, 1:2]) ** 2) / discs[:, 0, 2:3] ** 2 - 1.0
        ok = st == 1
        print(json.dumps({'leg': 'keepout', 'B': B, 'nodes': N, 'entry': what, 'seconds_median': med[what], 'seconds_min': min(times[what][1:]),
                          'seconds_max': max(times[what][1:]), 'problems_per_s': B / med[what], 'keepout_over_plain': med['keepout'] / med['plain'],
                          'status_counts': {int(k): int((st == k).sum()) for k in np.unique(st)}, 'mean_newton_steps': float(it.mean()),
                          'max_newton_steps': int(it.max()), 'mean_newton_steps_converged': float(it[ok].mean()) if ok.any() else None,
                          'min_g_over_R2_converged': float(g[ok].min()) if ok.any() else None,
                          'plans_inside_the_disc': int((g[ok].min(axis=1) < 0).sum()) if ok.any() else None}), flush=True)
    ctx.close()


def keepout_free_leg(B):
    import torch, d2dhip
    import d2dhip as D
    from d2dhip import synth
    from d2d.opty_utils import KeepOut
    ctx = d2dhip.Context(0)
    rows, W0, h = synth.nlp_problems(B)
    N = W0.shape[2]
    p0, p1 = rows[:, D.SC_X0:D.SC_X0 + 2], rows[:, D.SC_X1:D.SC_X1 + 2]
    d = p1 - p0
    d /= np.hypot(d[:, 0], d[:, 1])[:, None]
    c = 0.5 * (p0 + p1) + 3.0 * np.stack([-d[:, 1], d[:, 0]], 1)
    tabs = {'fixed': np.array([[KeepOut(c[b], 15.0).lowered(rows[b, D.SC_VMAX], h)] for b in range(B)])}
    tabs['free'] = tabs['fixed']
    tabs['free_hhi'] = np.array([[KeepOut(c[b], 15.0).lowered(rows[b, D.SC_VMAX], 2.0 * h)] for b in range(B)])
    dsc = ctx.dev(rows)
    dk = {k: ctx.dev(v) for k, v in tabs.items()}
    fr = ctx.dev(np.tile([0.5 * h, 2.0 * h, 0.0, 0.0], (B, 1)))
    names = ('fixed', 'free', 'free_hhi')
    times = {k: [] for k in names}
    outs, Ws = {}, {}
    for rep in range(6):                                     # the first launch of each is the warm-up; the entries alternate
        for what in names:
            W = ctx.dev(np.ascontiguousarray(W0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            outs[what] = ctx.nlp_solve_keepout(dsc, W, h, dk[what]) if what == 'fixed' else ctx.nlp_solve_free_fence(dsc, W, h, fr, discs=dk[what])
            e1.record(); torch.cuda.synchronize()
            times[what].append(e0.elapsed_time(e1) * 1e-3)
            Ws[what] = W
    med = {k: float(np.median(v[1:])) for k, v in times.items()}
    st = {k: outs[k]['status'].cpu().numpy() for k in names}
    for what in names:
        it = outs[what]['iters'].cpu().numpy()
        Wh, discs = Ws[what].cpu().numpy(), tabs[what]
        g = ((Wh[:, 0, 1:-1] - discs[:, 0, 0:1]) ** 2 + (Wh[:, 1, 1:-1] - discs[:, 0, 1:2]) ** 2) / discs[:, 0, 2:3] ** 2 - 1.0
        ok = st[what] == 1
        rec = {'leg': 'keepout-free', 'B': B, 'nodes': N, 'entry': what, 'seconds_median': med[what], 'seconds_min': min(times[what][1:]),
               'seconds_max': max(times[what][1:]), 'problems_per_s': B / med[what], 'problems_per_s_min_max': [B / max(times[what][1:]), B / min(times[what][1:])],
               'over_fixed': med[what] / med['fixed'], 'status_counts': {int(k): int((st[what] == k).sum()) for k in np.unique(st[what])},
               'mean_newton_steps': float(it.mean()), 'max_newton_steps': int(it.max()),
               'mean_newton_steps_converged': float(it[ok].mean()) if ok.any() else None,
               'min_g_over_R2_converged': float(g[ok].min()) if ok.any() else None}
        if what != 'fixed':
            hh = outs[what]['h'].cpu().numpy()
            rec.update(fixed_not_converged=int((st['fixed'] != 1).sum()), of_those_free_converged=int((ok & (st['fixed'] != 1)).sum()),
                       fixed_converged_free_not=int((~ok & (st['fixed'] == 1)).sum()),
                       duration_min_mean_max=[float(v) * (N - 1) for v in (hh[ok].min(), hh[ok].mean(), hh[ok].max())] if ok.any() else None)
        print(json.dumps(rec), flush=True)
    ctx.close()


def fence_leg(B):
    import torch, d2dhip
    import d2dhip as D
    from d2dhip import synth
    from d2d.opty_utils import KeepOut, GeoFence
    ctx = d2dhip.Context(0)
    rows, W0, h = synth.nlp_problems(B)
    N = W0.shape[2]
    p0, p1 = rows[:, D.SC_X0:D.SC_X0 + 2], rows[:, D.SC_X1:D.SC_X1 + 2]
    d = p1 - p0
    ll = np.hypot(d[:, 0], d[:, 1])
    d /= ll[:, None]
    nrm = np.stack([-d[:, 1], d[:, 0]], 1)
    c = 0.5 * (p0 + p1) + 3.0 * nrm
    discs = np.array([[KeepOut(c[b], 15.0).lowered(rows[b, D.SC_VMAX], h)] for b in range(B)])
    dsc, dk = ctx.dev(rows), ctx.dev(discs)
    Wf = ctx.dev(np.ascontiguousarray(W0))
    ctx.nlp_solve(dsc, Wf, h)                                # the free plans: where each leaves its leg's axis most
    ctx.sync()
    Wf = Wf.cpu().numpy()
    lat = (Wf[:, 0] - p0[:, 0:1]) * nrm[:, 0:1] + (Wf[:, 1] - p0[:, 1:2]) * nrm[:, 1:2]
    up = lat.max(1) >= -lat.min(1)
    cut = np.maximum(0.8 * np.abs(lat).max(1), 0.05)         # (half of it is infeasible for these legs: 4095 of 4096 end STALLED)
    left, right = np.where(up, cut, ll), np.where(up, ll, cut)
    edges = np.stack([GeoFence([p0[b] - 0.5 * ll[b] * d[b] - right[b] * nrm[b], p1[b] + 0.5 * ll[b] * d[b] - right[b] * nrm[b],
                                p1[b] + 0.5 * ll[b] * d[b] + left[b] * nrm[b], p0[b] - 0.5 * ll[b] * d[b] + left[b] * nrm[b]]).lowered() for b in range(B)])
    de, dz = ctx.dev(edges), ctx.dev(np.zeros_like(edges))
    names = ('keepout', 'fence', 'fence-absent')
    times = {k: [] for k in names}
    outs, Ws = {}, {}
    for rep in range(6):                                     # the first launch of each is the warm-up; the entries alternate
        for what in names:
            W = ctx.dev(np.ascontiguousarray(W0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            outs[what] = ctx.nlp_solve_keepout(dsc, W, h, dk) if what == 'keepout' else (ctx.nlp_solve_fence(dsc, W, h, de) if what == 'fence' else ctx.nlp_solve_fence(dsc, W, h, dz, discs=dk))
            e1.record(); torch.cuda.synchronize()
            times[what].append(e0.elapsed_time(e1) * 1e-3)
            Ws[what] = W
    med = {k: float(np.median(v[1:])) for k, v in times.items()}
    same = bool(torch.equal(Ws['keepout'], Ws['fence-absent']) and torch.equal(outs['keepout']['iters'], outs['fence-absent']['iters'])
                and torch.equal(outs['keepout']['keep_mult'], outs['fence-absent']['keep_mult']))
    for what in names:
        st = outs[what]['status'].cpu().numpy(); it = outs[what]['iters'].cpu().numpy()
        Wh = Ws[what].cpu().numpy()
        g = edges[:, :, 2, None] - (edges[:, :, 0, None] * Wh[:, None, 0, 1:-1] + edges[:, :, 1, None] * Wh[:, None, 1, 1:-1])
        ok = st == 1
        zf = outs['fence']['fence_mult'].cpu().numpy()
        print(json.dumps({'leg': 'fence', 'B': B, 'nodes': N, 'entry': what, 'seconds_median': med[what], 'seconds_min': min(times[what][1:]),
                          'seconds_max': max(times[what][1:]), 'problems_per_s': B / med[what], 'over_keepout': med[what] / med['keepout'],
                          'status_counts': {int(k): int((st == k).sum()) for k in np.unique(st)}, 'mean_newton_steps': float(it.mean()),
                          'max_newton_steps': int(it.max()), 'mean_newton_steps_converged': float(it[ok].mean()) if ok.any() else None,
                          'min_g_at_the_edges_converged': float(g[ok].min()) if ok.any() else None,
                          'plans_whose_edge_dual_exceeds_1e-3': int((zf[ok].max(axis=(1, 2)) > 1e-3).sum()) if what == 'fence' and ok.any() else None,
                          'absent_edges_are_the_keepout_entry_bit_for_bit': same}), flush=True)
    ctx.close()


def keepout_moving_leg(B):
    import torch, d2dhip
    import d2dhip as D
    from d2dhip import synth
    from d2d.opty_utils import KeepOut, MovingKeepOut, lower_keep_moving
    ctx = d2dhip.Context(0)
    rows, W0, h = synth.nlp_problems(B)
    N = W0.shape[2]
    T = (N - 1) * h
    p0, p1 = rows[:, D.SC_X0:D.SC_X0 + 2], rows[:, D.SC_X1:D.SC_X1 + 2]
    d = p1 - p0
    d /= np.hypot(d[:, 0], d[:, 1])[:, None]
    nrm = np.stack([-d[:, 1], d[:, 0]], 1)
    c = 0.5 * (p0 + p1) + 3.0 * nrm
    discs = np.array([[KeepOut(c[b], 15.0).lowered(rows[b, D.SC_VMAX], h)] for b in range(B)])
    still = [lower_keep_moving([KeepOut(c[b], 15.0)], rows[b, D.SC_VMAX], h) for b in range(B)]
    cross = [lower_keep_moving([MovingKeepOut((-1.0, T + 1.0), (c[b] - 3.0 * nrm[b] * (0.5 * T + 1.0), c[b] + 3.0 * nrm[b] * (0.5 * T + 1.0)), 15.0)],
                               rows[b, D.SC_VMAX], h) for b in range(B)]
    tabs = {k: (ctx.dev(np.stack([t[0] for t in v])), ctx.dev(np.stack([t[1] for t in v]))) for k, v in (('still', still), ('crossing', cross))}
    dsc, dk = ctx.dev(rows), ctx.dev(discs)
    names = ('static', 'still', 'crossing')
    times = {k: [] for k in names}
    outs, Ws = {}, {}
    for rep in range(6):                                     # the first launch of each is the warm-up; the entries alternate
        for what in names:
            W = ctx.dev(np.ascontiguousarray(W0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            outs[what] = ctx.nlp_solve_keepout(dsc, W, h, dk) if what == 'static' else ctx.nlp_solve_keepout_moving(dsc, W, h, *tabs[what], t_start=0.0)
            e1.record(); torch.cuda.synchronize()
            times[what].append(e0.elapsed_time(e1) * 1e-3)
            Ws[what] = W
    med = {k: float(np.median(v[1:])) for k, v in times.items()}
    same = bool(torch.equal(Ws['static'], Ws['still']) and torch.equal(outs['static']['iters'], outs['still']['iters'])
                and torch.equal(outs['static']['keep_mult'], outs['still']['keep_mult']))
    for what in names:
        st = outs[what]['status'].cpu().numpy(); it = outs[what]['iters'].cpu().numpy()
        Wh = Ws[what].cpu().numpy()
        ctr = outs[what]['mov_work'].cpu().numpy()[:, 0] if what != 'static' else np.repeat(discs[:, 0, :2, None], N, axis=2)
        R = discs[:, 0, 2] if what != 'crossing' else tabs['crossing'][1].cpu().numpy()[:, 0, 0]
        g = ((Wh[:, 0, 1:-1] - ctr[:, 0, 1:-1]) ** 2 + (Wh[:, 1, 1:-1] - ctr[:, 1, 1:-1]) ** 2) / R[:, None] ** 2 - 1.0
        ok = st == 1
        print(json.dumps({'leg': 'keepout-moving', 'B': B, 'nodes': N, 'entry': what, 'seconds_median': med[what], 'seconds_min': min(times[what][1:]),
                          'seconds_max': max(times[what][1:]), 'problems_per_s': B / med[what], 'over_static': med[what] / med['static'],
                          'status_counts': {int(k): int((st == k).sum()) for k in np.unique(st)}, 'mean_newton_steps': float(it.mean()),
                          'max_newton_steps': int(it.max()), 'mean_newton_steps_converged': float(it[ok].mean()) if ok.any() else None,
                          'min_g_over_R2_converged': float(g[ok].min()) if ok.any() else None,
                          'still_track_is_the_static_entry_bit_for_bit': same}), flush=True)
    ctx.close()


def guess_leg(B):
    import time
    import torch, d2dhip
    from d2dhip import synth
    from d2d.opty_utils import triangle
    ctx = d2dhip.Context(0)
    rows, W0, h = synth.nlp_problems(B)
    N = W0.shape[2]
    dsc = ctx.dev(rows)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        r = fn()
        e1.record(); torch.cuda.synchronize()
        return r, e0.elapsed_time(e1) * 1e-3

    # the host dog-leg and its copy: what the device start replaces (wall clock, the loop of synth.nlp_problems on the same end poses)
    host = []
    for rep in range(3):
        t0 = time.perf_counter()
        Wh = np.stack([np.stack(triangle(r[d2dhip.SC_X0:d2dhip.SC_X0 + 2], r[d2dhip.SC_X1:d2dhip.SC_X1 + 2], 12., 12.0, N, go_left=-1.), 0) for r in rows])
        ctx.dev(Wh); torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
    assert np.array_equal(Wh, W0)
    kern = {}
    for Bk in sorted({B, 65536}):
        big = ctx.dev(np.ascontiguousarray(np.tile(rows, (-(-Bk // B), 1))[:Bk]))
        Wk = ctx.empty(Bk, 5, N)
        ts = [timed(lambda: ctx.nlp_guess_dubins(big, N, h, W=Wk))[1] for rep in range(6)]
        kern[Bk] = dict(seconds_median=float(np.median(ts[1:])), seconds_min=min(ts[1:]), seconds_max=max(ts[1:]))
    print(json.dumps({'leg': 'guess', 'what': 'start alone', 'nodes': N, 'host_dogleg_and_copy_seconds': {'B': B, 'min': min(host), 'max': max(host)},
                      'guess_kernel': kern}), flush=True)
    times = {'dogleg': [], 'dubins': []}
    outs, gst = {}, None
    for rep in range(6):                                     # the first launch of each is the warm-up; the starts alternate
        for what in ('dogleg', 'dubins'):
            if what == 'dogleg':
                W = ctx.dev(np.ascontiguousarray(W0))
            else:
                W, g = ctx.nlp_guess_dubins(dsc, N, h)
                gst = g['status']
            outs[what], t = timed(lambda: ctx.nlp_solve(dsc, W, h))
            times[what].append(t)
    med = {k: float(np.median(v[1:])) for k, v in times.items()}
    st = {k: o['status'].cpu().numpy() for k, o in outs.items()}
    both = (st['dogleg'] == 1) & (st['dubins'] == 1)
    dc = np.abs(outs['dogleg']['cost'].cpu().numpy() - outs['dubins']['cost'].cpu().numpy())
    gs = gst.cpu().numpy()
    for what in ('dogleg', 'dubins'):
        it = outs[what]['iters'].cpu().numpy()
        ok = st[what] == 1
        print(json.dumps({'leg': 'guess', 'B': B, 'nodes': N, 'start': what, 'seconds_median': med[what], 'seconds_min': min(times[what][1:]),
                          'seconds_max': max(times[what][1:]), 'problems_per_s': B / med[what], 'dubins_over_dogleg': med['dubins'] / med['dogleg'],
                          'status_counts': {int(k): int((st[what] == k).sum()) for k in np.unique(st[what])}, 'mean_newton_steps': float(it.mean()),
                          'max_newton_steps': int(it.max()), 'mean_newton_steps_converged': float(it[ok].mean()) if ok.any() else None,
                          'same_status_as_the_other_start': int((st['dogleg'] == st['dubins']).sum()), 'converged_from_both': int(both.sum()),
                          'largest_cost_difference_converged_from_both': float(dc[both].max()) if both.any() else None,
                          'guess_status_counts': {d2dhip.GUESS_STATUS[int(k)]: int((gs == k).sum()) for k in np.unique(gs)}}), flush=True)
    ctx.close()


def main():
    if sys.argv[1:2] == ['guess']:
        return guess_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    if sys.argv[1:2] == ['fence']:
        return fence_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    if sys.argv[1:2] == ['keepout-moving']:
        return keepout_moving_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    if sys.argv[1:2] == ['keepout-free']:
        return keepout_free_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    if sys.argv[1:2] == ['keepout']:
        return keepout_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    if sys.argv[1:2] == ['free']:
        return free_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    if sys.argv[1:2] == ['via']:
        return via_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    if sys.argv[1:2] == ['moving']:
        return moving_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    if sys.argv[1:2] == ['pairs']:
        return pairs_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
    if sys.argv[1:2] == ['groups']:
        return groups_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
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
