"""Writes tests/golden/fit_terminal_starts.npz: the twelve fits per (plan, mode) that tests/test_fit_terminal_cpu.py and
tests/test_gpu_fit_terminal.py run under a trial cap of 1, 2 and 5 and compare with the oracle one by one.

A capped fit stops mid-path, and mid-path the iterates of a fit started at the 'tri' guess depend on the rounding of the fp32 Hessian at
the 1e-5 level (the oracle's own fp32 split against its fp64 statement) -- no kernel can be held to 1e-6 there.  So the fits start
NEAR a minimum: a scenario row of the plan's bench-style batch, its minimiser by the oracle (fp64, uncapped), and a start point
q* + sigma max|q*| N(0, 1) with sigma cycling through 1e-2 .. 1e-7 -- far enough that the cap stops most of them, near enough that
some converge within five trials.  Of a pool of such fits the first twelve are kept on which the oracle's fp32 split and its fp64
statement agree within 1e-7 (1e-8 for the long-horizon plan: MARGINS) in status, cost and q under every cap: ten times inside
the tolerance the tests ask of the kernels.  The choice uses the oracle alone.

    python tests/golden/make_fit_terminal_golden.py        (CPU, about a minute)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'drone-sim-python_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import fit_terminal_ref as R                      # noqa: E402
from oracle import fit as F, fit_knot as FK       # noqa: E402

POOL = 96
SIGMAS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7)
MARGIN = 1e-7
# the long-horizon kernel forms its fp32 Hessian in two fp32 stages -- per-segment blocks on the matrix cores, then their projection
# through the fp32 Legendre tables (csrc/fit_seg.h) -- where the oracle's split rounds an fp64 Hessian once: its fits are chosen
# another factor of ten inside
MARGINS = {'long65': 1e-8}


def main():
    out = {}
    for name, mode in R.CASES:
        basis = R.oracle_basis(name)
        kb = FK.KnotBasis(basis) if R.PLANS[name][3] == 'knot' else None
        sc = R.scenarios(name, POOL)
        rng = np.random.default_rng(20241008)
        rows, starts, n_conv = [], [], 0
        for i in range(POOL):
            qs, _, _, st = R.oracle_solve(name, mode, basis, sc[i], F.initial_guess(basis, sc[i]), 200, False, kb)
            q0 = qs + SIGMAS[i % len(SIGMAS)] * np.abs(qs).max() * rng.standard_normal(len(qs))
            if st != F.ST_CONVERGED:
                continue
            ok, conv5 = True, False
            for cap in R.CAPS:
                a = R.oracle_solve(name, mode, basis, sc[i], q0, cap, True, kb)
                b = R.oracle_solve(name, mode, basis, sc[i], q0, cap, False, kb)
                ok = ok and R.agree(a, b, MARGINS.get(name, MARGIN))
                conv5 = cap == 5 and a[3] == F.ST_CONVERGED
            if not ok or (conv5 and n_conv >= 6):       # (at most half of the sample may converge: the cap must stop the rest)
                continue
            n_conv += int(conv5)
            rows.append(sc[i]); starts.append(q0)
            if len(rows) == 12:
                break
        assert len(rows) == 12, (name, mode, len(rows))
        assert 1 <= n_conv <= 8, (name, mode, n_conv)
        print(name, mode, 'pool used', i + 1, 'converge within 5 trials:', n_conv)
        out['%s_%s_rows' % (name, mode)] = np.array(rows)
        out['%s_%s_q0' % (name, mode)] = np.array(starts)
    np.savez(os.path.join(HERE, 'fit_terminal_starts.npz'), **out)


if __name__ == '__main__':
    main()
