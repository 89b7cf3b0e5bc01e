"""Generator of tests/golden/nlp_free_slsqp.npz: an arbiter of the free-time-step collocation solve that shares nothing with the solver
(csrc/nlp_kernels.hip d2d_nlp_solve_free) or its CPU statement (tests/nlp_free_ref.py) but the problem.

scipy's SLSQP minimises, over the free node values and the interval h itself (NOT u = 1 / h),

    objective(W) + k_dur (N - 1) h    subject to   the backward-Euler equalities in the reference's form at h,   the boxes, h_lo <= h <= h_hi

with analytic gradients (oracle.nlp.cost_grad; the Jacobian of the equalities written out below), ftol 1e-12, from the same start as
the solver.  The end conditions are not variables.  Cases: 5, 9 and 17 nodes, k_dur > 0 so that h is determined; two of them round a
kind-1 disc, one has a y box (the objective minimised is the one whose gradient is the reference's cost_grad, oracle/nlp.py; the cost stored is the
reference's cost() + k_dur (N - 1) h at the minimiser, like the solver's).  Stored per case: the scenario row, the row of the step's
box, the start, and SLSQP's cost, h, feasibility, iteration count and W.

Run from the repository root:  python tests/golden/make_nlp_free_golden.py
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'drone-sim-python_amd')]

import nlp_free_ref as F          # noqa: E402  (the problems only: leg_problem)
from oracle import nlp            # noqa: E402

CASES = ((5, 0, dict(k_dur=0.5, obj_scale=1.25)), (9, 0, dict(k_dur=2.0, box=True)), (9, 1, dict(k_dur=0.5, obstacle=1)),
         (17, 0, dict(k_dur=0.5, obstacle=1)), (17, 1, dict(k_dur=0.5)))


def slsqp(fp, W0, h_start):
    pb = fp.pb
    N = pb.N
    fixed = pb.lo == pb.hi
    free = ~fixed
    Wf = np.where(fixed, pb.lo, W0)
    lo, hi = pb.lo[free], pb.hi[free]
    kd = fp.k_dur * (N - 1)

    def unpack(z):
        W = Wf.copy()
        W[free] = z[:-1]
        return W, z[-1]

    def fun(z):
        W, h = unpack(z)
        return nlp.objective(pb, W) + kd * h

    def grad(z):
        W, h = unpack(z)
        return np.concatenate([nlp.cost_grad(pb, W)[free], [kd]])

    def con(z):
        W, h = unpack(z)
        return nlp.constraints(fp.at(1.0 / h), W).reshape(-1)

    def jac(z):
        W, h = unpack(z)
        x, y, psi, phi, v = W.T
        J = np.zeros((N - 1, 3, N, 5)); Jh = np.zeros((N - 1, 3))
        for i in range(1, N):
            k = i - 1
            for c in range(3):
                J[k, c, i, c] += 1.0 / h; J[k, c, i - 1, c] -= 1.0 / h
                Jh[k, c] = -(W[i, c] - W[i - 1, c]) / (h * h)
            J[k, 0, i, 2] += v[i] * np.sin(psi[i]); J[k, 0, i, 4] += -np.cos(psi[i])
            J[k, 1, i, 2] += -v[i] * np.cos(psi[i]); J[k, 1, i, 4] += -np.sin(psi[i])
            J[k, 2, i, 3] += -nlp.G_ACC / v[i] / np.cos(phi[i]) ** 2; J[k, 2, i, 4] += nlp.G_ACC * np.tan(phi[i]) / v[i] ** 2
        return np.concatenate([J.reshape(3 * (N - 1), N, 5)[:, free], Jh.reshape(-1, 1)], 1)

    z0 = np.concatenate([np.clip(Wf[free], lo + 1e-3 * np.where(np.isfinite(hi - lo), hi - lo, 1.0), hi - 1e-3 * np.where(np.isfinite(hi - lo), hi - lo, 1.0)), [h_start]])
    bounds = [(a if np.isfinite(a) else None, b if np.isfinite(b) else None) for a, b in zip(lo, hi)] + [(fp.h_lo, fp.h_hi)]
    res = minimize(fun, z0, jac=grad, bounds=bounds, constraints=[dict(type='eq', fun=con, jac=jac)], method='SLSQP',
                   options=dict(ftol=1e-12, maxiter=500))
    W, h = unpack(res.x)
    return W, h, res


def main():
    out = {}
    for k, (N, seed, kw) in enumerate(CASES):
        fp, row, W0 = F.leg_problem(N, 900 + seed, **kw)
        W, h, res = slsqp(fp, W0, F.H0)
        cost, feas = fp.cost(W, 1.0 / h), float(np.abs(fp.constraints(W, 1.0 / h)).max())
        print(f'case {k}: N {N} {kw}: {res.message!r} after {res.nit} iterations, cost {cost:.12f}, h {h:.12f}, feas {feas:.2e}')
        assert res.success and feas <= 1e-9 and fp.h_lo < h < fp.h_hi
        out.update({f'c{k}_N': N, f'c{k}_row': row, f'c{k}_free_row': np.array([fp.h_lo, fp.h_hi, fp.k_dur, 0.0]), f'c{k}_W0': W0, f'c{k}_W': W,
                    f'c{k}_cost': cost, f'c{k}_h': h, f'c{k}_feas': feas, f'c{k}_nit': res.nit})
    out['n_cases'] = len(CASES)
    np.savez_compressed(os.path.join(HERE, 'nlp_free_slsqp.npz'), **out)


if __name__ == '__main__':
    main()
