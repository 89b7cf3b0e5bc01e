"""(CPU) One SHA-256 per case over what the CPU statements of the collocation solver return (oracle/nlp.py, tests/nlp_*_ref.py): the
check that a change to their code changed no bit of their results.  Run it on two trees with the same Python, numpy and BLAS and
compare the outputs with diff:

    python tools/dev/nlp_ref_digest.py > after.txt;   cp tools/dev/nlp_ref_digest.py OTHER_TREE/tools/dev/;  (there) ... > before.txt

The digests depend on the host's BLAS and libm: they are compared between trees on one machine, never committed.  Only the statements'
entry points (solve, solve_groups, solve_moving) and their case builders are used, so the script runs on a tree from before the loops
were folded into oracle.nlp.solve_general as it does after.

A digest covers W and every entry of info in the order of the sorted keys: arrays as raw float64 bytes, scalars as float64 or int64,
`path` and other sequences as float64 arrays; a nested info (the step cases' `raw`) key by key in the same way.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import nlp_fence_ref as F                 # noqa: E402
import nlp_free_ref as FR                 # noqa: E402
import nlp_keepout_moving_ref as KM       # noqa: E402
import nlp_keepout_ref as K               # noqa: E402
import nlp_steps_ref as S                 # noqa: E402
import nlp_via_ref as V                   # noqa: E402
import nlp_wind_ref as R                  # noqa: E402

BUDGETS = ((8, 1), (5, 4))                # (inner_max, outer_max) of the step cases: one outer iteration, and the schedule moving


def feed(h, v):
    if isinstance(v, dict):
        for k in sorted(v):
            h.update(k.encode())
            feed(h, v[k])
    elif isinstance(v, (bool, int, np.integer)):
        h.update(np.int64(v).tobytes())
    elif isinstance(v, (float, np.floating)):
        h.update(np.float64(v).tobytes())
    else:                                 # arrays, path (a list of tuples), tuples of scalars
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())


def emit(name, W, info):
    h = hashlib.sha256()
    feed(h, np.asarray(W, float))
    feed(h, info)
    print(f'{h.hexdigest()}  {name}', flush=True)


def emit_groups(name, got):
    Ws, infos, sweeps, moved = got
    emit(name, np.stack(Ws), dict(infos={f'{a:02d}': i for a, i in enumerate(infos)}, sweeps=sweeps, moved=moved))


def steps(name, case):
    for b in BUDGETS:
        emit(f'{name} budget={b[0]}x{b[1]}', *case.run(case.W0, *b))


def main():
    for lid in S.launch_ids():
        for case in S.launch(lid).cases:
            steps(f'steps/{lid}/{case.cid}', case)
    # hard static discs
    for N in (17, 41):
        for tag, got in K.steps_launch(N).items():
            steps(f'keepout/steps-{N}-{tag}', got[0])
        for b, (prob, _, W0, discs, _) in enumerate(K.full_launch(N)):
            emit(f'keepout/full-{N}-{b}', *K.solve(prob, W0, discs))
    for N in K.ARB_N:
        for two in (False, True):
            pb, _, W0, discs = K.arbiter_problem(N, two)
            emit(f'keepout/arbiter-{N}-{int(two)}', *K.solve(K.Plain(pb), W0, discs))
    pb, _, W0, discs = K.arbiter_problem(17, False)
    emit('keepout/refused-p0-inside', *K.solve(K.Plain(pb), W0, np.array([(pb.p0[0], pb.p0[1], 1.0)])))
    # hard moving discs
    for N in (17, 41):
        for tag, got in KM.steps_launch(N).items():
            steps(f'keepmov/steps-{N}-{tag}', got[0])
        for b, (prob, _, W0, trs, _) in enumerate(KM.full_launch(N)):
            emit(f'keepmov/full-{N}-{b}', *KM.solve_moving(prob.pb, W0, trs, KM.FULL_T_START))
    for N in KM.ARB_N:
        for kind in KM.ARB_KINDS:
            pb, _, W0, trs = KM.arbiter_problem(N, kind)
            emit(f'keepmov/arbiter-{N}-{kind}', *KM.solve_moving(pb, W0, trs, KM.ARB_T_START))
    for N in KM.GROUP_N:
        rows, W0s, trs = KM.pair_scenario(N)
        emit_groups(f'keepmov/pair-{N}', KM.solve_groups(rows, trs, W0s, t_start=KM.GROUP_T_START, max_sweeps=KM.GROUP_SWEEPS, N=N, h=KM.H0))
    pb, _, W0, discs = K.arbiter_problem(17, False)
    emit('keepmov/refused-p1-inside', *KM.solve(KM.Plain(pb), W0, *KM.constant_centres([(pb.p1[0], pb.p1[1], 1.0)], 17)))
    # the fence
    for N in (17, 41):
        for tag, got in F.steps_launch(N).items():
            steps(f'fence/steps-{N}-{tag}', got[0])
        for b, (prob, _, W0, discs, edges, _) in enumerate(F.full_launch(N)):
            emit(f'fence/full-{N}-{b}', *F.solve(prob, W0, discs, edges))
    for name in F.ARB_CASES:
        pb, _, W0, discs, edges = F.arbiter_problem(name)
        emit(f'fence/arbiter-{name}', *F.solve(F.Plain(pb), W0, discs, edges))
    for N in F.GROUP_N:
        rows, W0s, edges = F.pair_scenario(N)
        emit_groups(f'fence/pair-{N}', F.solve_groups(rows, edges, W0s, max_sweeps=F.GROUP_SWEEPS, N=N, h=F.H0))
    pb, _, W0, discs, edges = F.arbiter_problem('cut-17')
    emit('fence/refused-kap-0', *F.solve(F.Plain(pb), W0, discs, edges * (1, 1, 1, 0)))
    # the free time step
    for N in FR.STEP_N:
        for case in FR.steps_launch(N)[0]:
            steps(f'free/{case.cid}', case)
    for case in FR.bounds_launch()[0]:
        steps(f'free/{case.cid}', case)
        emit(f'free/{case.cid} full', *case.run(case.W0, K.nlp.INNER_MAX, K.nlp.OUTER_MAX))
    # timed waypoints
    for wind in ('const', 'gust'):
        field, t0 = (None, 0.0) if wind == 'const' else (R.fields()['gust'], V.GUST_T_START)
        for name, (r, tab) in V.catalogue(wind).items():
            emit(f'via/{name}', *V.solve(V.problem(r, tab), V.guess(r, tab), field, t0))


if __name__ == '__main__':
    main()
