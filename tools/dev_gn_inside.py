#!/usr/bin/env python3
"""(CPU, oracle) Round 7, item 5 of the pass over the knot kernel's solver loop: would a LAZY ||L^-1 (M p / ||p||)||^2 after the
Gauss-Newton solve pay?  lmpar needs that forward substitution only when the Gauss-Newton step leaves the trust region -- at once, or
later, when a rejected trial has shrunk the region while the cached step of the same point is reused; the factor is gone by then (the
trial's evaluation overwrites the image), so a lazy version repeats the lambda = 0 factorisation.  Counted on the first n bench
scenarios with oracle/fit_knot.py solve_minpack_knot (fp32 Hessian and Cholesky, max_iter = 150):
  gn          Gauss-Newton solves (one per evaluated point)
  gn_inside   ... whose step lies inside the region: substitutions a lazy version skips
  reneeded    ... of those, later found too long for the shrunk region: factorisations a lazy version repeats
    python tools/dev_gn_inside.py [n=1024]"""
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'drone-sim-python_amd')]

import numpy as np  # noqa: E402

import bench  # noqa: E402
from oracle import fit as F, fit_knot as FK  # noqa: E402

_lmpar = FK.lmpar_knot
C = {}


def _counted(kb, H, g, delta, par, chol_dtype=np.float64):
    r = _lmpar(kb, H, g, delta, par, chol_dtype)
    inside = r[1] == 0.0 and r[2] == 1                  # returned from the Gauss-Newton step: par = 0 after ONE factorisation
    C['lmpar'] = C.get('lmpar', 0) + 1
    if C.get('H') is not H:                             # a new point: lmder evaluates H once per accepted step
        C['H'], C['lazy'] = H, inside
        C['gn'] = C.get('gn', 0) + 1
        C['gn_inside'] = C.get('gn_inside', 0) + int(inside)
    elif not inside and C['lazy']:
        C['reneeded'] = C.get('reneeded', 0) + 1
        C['lazy'] = False
    return r


def _one(i):
    C.clear()
    FK.lmpar_knot = _counted
    FK.solve_minpack_knot(KB, SC[i], hess_dtype=np.float32, chol_dtype=np.float32, max_iter=150)
    return {k: v for k, v in C.items() if k not in ('H', 'lazy')}


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    dur, wref = bench._plan_consts()
    KB = FK.KnotBasis(F.FitBasis(bench.S_, bench.K, dur, wref))
    SC = bench.bench_scenarios(4096)[:n]
    with mp.get_context('fork').Pool(min(16, os.cpu_count())) as pool:
        res = pool.map(_one, range(n), chunksize=8)
    tot = {}
    for r in res:
        for k, v in r.items():
            tot[k] = tot.get(k, 0) + v
    print(n, 'fits:', tot)
