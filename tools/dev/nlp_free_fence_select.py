"""(CPU) The selection behind tests/nlp_free_fence_ref.py's STEP_CASES and FULL_CASES, with the statement alone:

    python tools/dev/nlp_free_fence_select.py steps [N ...]     one line per cell (node count, kind): the chosen (radius, seed) or what fails
    python tools/dev/nlp_free_fence_select.py full [N ...]      eight full solves per node count

steps: the rule written above nlp_keepout_ref.STEP_CASES.  Per cell the radii 9, 8, 7, 6, 5 % of the leg, largest first ('edge' and 'many'
hold no disc that binds: one radius), and per radius the seeds 0 .. 15: the first candidate that nlp_steps_ref.check passes after every
budget of nlp_steps_ref.BUDGETS (nlp_free_fence_ref.step_complaints: at 3 and 5 nodes the budget (8, 1) is held to the tolerance and the
path alone, as the rule says) and whose largest dual over the budgets reaches 1 ('many', where nothing can bind: not asked).  A candidate is screened with its unperturbed run
first (the statuses, the counted steps, the dual), so that most of them cost 8 solves and not 72.
full: candidates in a fixed order; one is taken when the statement CONVERGES with h strictly inside its box, the 8 starts of
nlp_steps_ref.starts converge to the same cost and h within 1e-9 relative, and a dual of a disc or an edge ends above 1e-4.
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import nlp_free_fence_ref as FF           # noqa: E402
import nlp_steps_ref as S                 # noqa: E402


def screen(case, N):
    """the unperturbed runs: every budget with outer_max = 1 ends at the iteration cap with every counted step accepted; -> largest dual"""
    zmax = 0.0
    for budget in S.BUDGETS:
        _, info = case.run(case.W0, *budget)
        raw = info['raw']
        if budget[1] == 1 and not (N <= 5 and budget == (8, 1)) and (info['status'] != (S.ST_MAXITER,) or len(info['path']) != sum(info['inner'])):
            return None
        if raw['status'] == FF.ST_NONFINITE:
            return None
        zmax = max(zmax, float(raw['zk'].max(initial=0.0)), float(raw['zf'].max(initial=0.0)))
    return zmax


def pick_step(cell):
    N, tag = cell
    radii = FF.STEP_RADII if tag in ('disc', 'both') else FF.STEP_RADII[:1]
    why = {}
    for Rf in radii:
        for seed in range(FF.STEP_SEEDS):
            cand = FF.step_candidate(N, tag, Rf, seed)
            if cand is None:
                why[(Rf, seed)] = 'no corridor'
                continue
            case = cand[0]
            zmax = screen(case, N)
            if zmax is None or not (zmax >= 1.0 or tag == 'many'):      # ('many': every present row is far away, nothing can bind)
                why[(Rf, seed)] = 'ends early' if zmax is None else f'dual {zmax:.2g}'
                continue
            S._measured.clear()
            bad = [f'{b}: {c}' for b in S.BUDGETS for c in FF.step_complaints(case, N, b)[:1]]
            if not bad:
                tol = max(S.measure(case, b)['tol'] for b in S.BUDGETS)
                return cell, (Rf, seed), f'dual {zmax:.3g}, largest tol {tol:.1e}'
            why[(Rf, seed)] = bad[0]
    return cell, None, '; '.join(f'{k}: {v}' for k, v in list(why.items())[-3:])


def full_candidates(N):
    for seed in range(12):
        for k_dur, Rf, half in ((0.0, 0.09, 0.3), (0.5, 0.09, 0.0), (0.0, 0.0, -1), (2.0, 0.07, 0.3)):
            yield seed, k_dur, Rf, half


def try_full(arg):
    N, cand = arg
    FF.FULL_CASES[N] = (cand,)
    FF.full_launch.cache_clear()
    try:
        fp, r, W0, discs, edges = FF.full_launch(N)[0]
    except ValueError:                     # (no corridor: the plan without tables did not converge)
        return arg, None
    W, info = FF.solve(fp, W0, FF.H0, discs, edges)
    if info['status'] != 1 or not fp.h_lo * 1.001 < info['h'] < fp.h_hi * 0.999:
        return arg, None
    z = max(float(info['zk'].max(initial=0.0)), float(info['zf'].max(initial=0.0)))
    if not z > 1e-4:
        return arg, None
    case = FF.steps_case(f'freefence-full-{N}-{cand}', fp, W0, discs, edges)
    for Wp in S.starts(case):
        ip = FF.solve(fp, Wp[0][:N], FF.H0, discs, edges)[1]
        if ip['status'] != 1 or abs(ip['cost'] - info['cost']) > 1e-9 * abs(info['cost']) or abs(ip['h'] - info['h']) > 1e-9 * info['h']:
            return arg, None
    return arg, (info['inner'], info['h'], z)


if __name__ == '__main__':
    what = sys.argv[1]
    Ns = [int(a) for a in sys.argv[2:]]
    with Pool(int(os.environ.get('JOBS', '7'))) as pool:
        if what == 'steps':
            cells = [(N, tag) for N in (Ns or FF.STEP_N) for tag in FF.STEP_TAGS]
            for cell, got, note in pool.imap_unordered(pick_step, sorted(cells, key=lambda c: -c[0])):
                print(f'{cell}: {got},   # {note}', flush=True)
        else:
            for N in Ns or FF.FULL_N:
                took = []
                for (_, cand), got in pool.imap(try_full, [(N, c) for c in full_candidates(N)]):
                    if got and len(took) < 8:
                        took.append(cand)
                        print(f'{N}: {cand},   # steps {got[0]}, h {got[1]:.5f}, largest dual {got[2]:.3g}', flush=True)
                print(f'FULL_CASES[{N}] = {tuple(took)}', flush=True)
