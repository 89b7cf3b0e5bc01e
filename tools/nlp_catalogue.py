#!/usr/bin/env python3
"""The collocation backend over the reference's single-aircraft scenario catalogue (d2d.optyplan_scenarios.scens, every case):
status, Newton steps, cost, feasibility -- a robustness survey of d2d_nlp_solve.  python tools/nlp_catalogue.py
--free-time: every case with its duration freed to [t / 2, 2 t] (t = t1 - t0; the scenario protocol's t1_free, d2d_nlp_solve_free):
status, duration and cost per case.  Cases that a free step is not combined with (a wind field, moving obstacles, waypoints, a host
cost) report the refusal.
--keep-out: every case with its soft discs (the cost's static obstacles) turned into hard ones (the scenario protocol's keep_out,
d2d_nlp_solve_keepout; no margin): status, cost and the polyline's clearance per disc.  Cases without a disc, and those a hard disc is not
combined with, say so.
--free-time --keep-out together: the cases that carry discs with the discs hard AND the duration free in [t / 2, 2 t] (the scenario
protocol's t1_window beside keep_out, d2d_nlp_solve_free_fence; the discs lowered for the largest step): status, duration, cost and
clearance per disc.
--guess dubins: every case from the device Dubins start (Planner.get_initial_guess('dubins'), d2d_nlp_guess_dubins) beside the case's
own start: verdict and Newton steps of both, the status of the guess, and the difference of the two costs.  Combines with --free-time."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd')):
    sys.path.insert(0, _p)
import numpy as np


def main():
    free = '--free-time' in sys.argv[1:]
    hard = '--keep-out' in sys.argv[1:]
    guess = sys.argv[sys.argv.index('--guess') + 1] if '--guess' in sys.argv[1:] else None
    if guess not in (None, 'dubins'):
        sys.exit(f"--guess {guess}: 'dubins' is the only start surveyed beside the case's own")
    import d2d.optyplan_scenarios as sc
    import single_opt_planner as sop
    # the reference's sweeps mutate exp_0 (exp_0_1: t1, exp_0_2: wind, exp_6: p0 / p1) and every exp_0-based scenario sees it:
    # restore exp_0 before each scenario, so that every scenario is surveyed as if it were the first one run
    keep = {k: getattr(sc.exp_0, k) for k in ('t1', 'wind', 'p0', 'p1')}
    for s in sc.scens:
        for k, v in keep.items():
            setattr(sc.exp_0, k, v)
        for case in range(s.ncases):
            s.set_case(case)
            try:
                exp = s
                if free:                                # the case as it stands, with t1 free in [t0 + t / 2, t0 + 2 t]
                    t = s.t1 - s.t0
                    exp = type(s.__name__ + '_free', (s,), {'t1_window' if hard else 't1_free': (s.t0 + 0.5 * t, s.t0 + 2.0 * t)})
                if hard:                                # the cost's own discs, held instead of priced (they stay in the cost as well)
                    from d2d.opty_utils import KeepOut
                    obss = sop.lower_cost(s.cost)[4]
                    if not obss:
                        print(json.dumps({'scen': s.name, 'case': case, 'keep_out': 'no disc in this case'}), flush=True)
                        continue
                    exp = type(exp.__name__ + '_hard', (exp,), {'keep_out': [KeepOut(o[:2], o[2]) for o in obss]})
                p = sop.Planner(exp, initialize=True, backend='nlp')
                t0 = time.perf_counter()
                p.run(p.get_initial_guess(getattr(s, 'initial_guess', 'tri')))
                dt = time.perf_counter() - t0
                rec = {'scen': s.name, 'case': case, 'nodes': p.num_nodes, 'status': p.info['status'], 'iters': p.info['iters'],
                       'cost': p.info['obj_val'], 'feas': p.info['feas'], 'seconds': round(dt, 3)}
                if free:
                    rec.update(duration=p.duration, asked=s.t1 - s.t0)
                if hard:
                    rec.update(discs=len(exp.keep_out), keep_out_clearance=p.info.get('keep_out_clearance'))
                if guess:                               # the same case from the Dubins start, beside the start it names
                    try:
                        q = sop.Planner(exp, initialize=True, backend='nlp')
                        g = q.get_initial_guess(guess)
                        q.run(g)
                        import d2dhip
                        rec.update(guess=[d2dhip.GUESS_STATUS[k] for k in q.guess_status], guess_status=q.info['status'], guess_iters=q.info['iters'],
                                   guess_cost_diff=q.info['obj_val'] - p.info['obj_val'])
                        if free:
                            rec.update(guess_duration=q.duration)
                    except (NotImplementedError, ValueError) as e:
                        rec.update(guess=f'{type(e).__name__}: {e}'[:160])
                print(json.dumps(rec), flush=True)
            except Exception as e:                      # noqa: BLE001 -- a survey: report and go on
                print(json.dumps({'scen': s.name, 'case': case, 'error': f'{type(e).__name__}: {e}'[:200]}), flush=True)


if __name__ == '__main__':
    main()
