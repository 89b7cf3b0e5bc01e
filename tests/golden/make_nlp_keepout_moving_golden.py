"""Generator of tests/golden/nlp_keepout_moving_slsqp.npz: an arbiter of the collocation solve with hard keep-out discs that MOVE that
shares nothing with the solver (csrc/nlp_kernels.hip d2d_nlp_solve_keepout_moving) or the loop of its CPU statement
(tests/nlp_keepout_moving_ref.py) but the problem, the sampled centres and the start.

scipy's SLSQP minimises, over the free node values,

    objective(W)   subject to   the backward-Euler equalities,   the boxes,   |p_i - c(t_i)|^2 - R^2 >= 0 at every interior node

with the node inequalities as TRUE constraints (type 'ineq', analytic Jacobians; the centres are data), ftol 1e-13, from the
statement's start rule applied to the same W0.  Cases (nlp_keepout_moving_ref.arbiter_problem): 5, 9 and 17 nodes; one disc that
crosses the leg, and one that overtakes the aircraft along it.  Stored per case: the scenario row, the track's knots and node radius,
the start time, W0, and SLSQP's cost (the reference's cost()), feasibility, smallest g, iteration count and W.

Measured when the file was made (the statement nlp_keepout_moving_ref.solve_moving against SLSQP, relative difference of the cost):
  N 5 cross 1.1e-09, overtake 1.2e-09;  N 9 cross 5.6e-10, overtake 8.3e-10;  N 17 cross 2.2e-09, overtake 9.4e-10
so the tests' cost tolerance is 10 x the largest: 2.2e-8 (tests/test_nlp_keepout_moving_cpu.py SLSQP_COST_RTOL).  Node values are not
compared: they are not unique in the flat directions of the objective.

Run from the repository root:  python tests/golden/make_nlp_keepout_moving_golden.py
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'drone-sim-python_amd')]

import nlp_keepout_moving_ref as KM       # noqa: E402  (the problems, the centres and the start rule only)
from oracle import nlp                    # noqa: E402

CASES = tuple((N, kind) for N in KM.ARB_N for kind in KM.ARB_KINDS)


def slsqp(pb, W0, ctr, R):
    N = pb.N
    fixed, hasL, hasU = nlp._barrier_sets(pb)
    free = ~fixed
    Wf = np.where(fixed, pb.lo, W0)
    Wf = np.where(hasL, np.maximum(Wf, pb.lo + 1e-2 * (pb.hi - pb.lo)), Wf)
    Wf = np.where(hasU, np.minimum(Wf, pb.hi - 1e-2 * (pb.hi - pb.lo)), Wf)
    Wf = KM.start(pb, Wf, ctr, R)
    lo, hi = pb.lo[free], pb.hi[free]
    pos = np.cumsum(free.reshape(-1)).reshape(free.shape) - 1          # index of a free variable in z
    ci = ctr[:, 1:-1]

    def unpack(z):
        W = Wf.copy()
        W[free] = z
        return W

    def con(z):
        return nlp.constraints(pb, unpack(z)).reshape(-1)

    def jac(z):
        W = unpack(z)
        x, y, psi, phi, v = W.T
        h = pb.h
        J = np.zeros((N - 1, 3, N, 5))
        for i in range(1, N):
            k = i - 1
            for c in range(3):
                J[k, c, i, c] += 1.0 / h; J[k, c, i - 1, c] -= 1.0 / h
            J[k, 0, i, 2] += v[i] * np.sin(psi[i]); J[k, 0, i, 4] += -np.cos(psi[i])
            J[k, 1, i, 2] += -v[i] * np.cos(psi[i]); J[k, 1, i, 4] += -np.sin(psi[i])
            J[k, 2, i, 3] += -nlp.G_ACC / v[i] / np.cos(phi[i]) ** 2; J[k, 2, i, 4] += nlp.G_ACC * np.tan(phi[i]) / v[i] ** 2
        return J.reshape(3 * (N - 1), N, 5)[:, free]

    def gfun(z):
        return KM.g_values(unpack(z)[1:-1], ci, R)[0].reshape(-1)

    def gjac(z):
        _, dx, dy = KM.g_values(unpack(z)[1:-1], ci, R)
        J = np.zeros((len(R), N - 2, len(z)))
        for m in range(len(R)):
            for i in range(1, N - 1):
                J[m, i - 1, pos[i, 0]] = 2.0 * dx[m, i - 1]; J[m, i - 1, pos[i, 1]] = 2.0 * dy[m, i - 1]
        return J.reshape(-1, len(z))

    bounds = [(a if np.isfinite(a) else None, b if np.isfinite(b) else None) for a, b in zip(lo, hi)]
    res = minimize(lambda z: nlp.objective(pb, unpack(z)), Wf[free], jac=lambda z: nlp.cost_grad(pb, unpack(z))[free], bounds=bounds,
                   constraints=[dict(type='eq', fun=con, jac=jac), dict(type='ineq', fun=gfun, jac=gjac)], method='SLSQP',
                   options=dict(ftol=1e-13, maxiter=1000))
    return unpack(res.x), res


def main():
    out = {}
    for k, (N, kind) in enumerate(CASES):
        pb, row, W0, trs = KM.arbiter_problem(N, kind)
        ctr, R = KM.centres(trs, KM.ARB_T_START, N, pb.h)
        W, res = slsqp(pb, W0, ctr, R)
        cost, feas = nlp.cost(pb, W), float(np.abs(nlp.constraints(pb, W)).max())
        gmin = float((KM.g_values(W[1:-1], ctr[:, 1:-1], R)[0] / R[:, None] ** 2).min())
        Ws, info = KM.solve_moving(pb, W0, trs, KM.ARB_T_START)
        print(f'case {k}: N {N}, {kind}: {res.message!r} after {res.nit} iterations, cost {cost:.12f}, feas {feas:.2e}, min g / R^2 {gmin:.2e}; '
              f'the statement: status {info["status"]}, cost {info["cost"]:.12f}, relative difference {abs(info["cost"] - cost) / cost:.1e}')
        assert res.success and feas <= 1e-9 and gmin >= -1e-9
        out.update({f'c{k}_N': N, f'c{k}_kind': kind, f'c{k}_row': row, f'c{k}_knots': trs[0].padded(2), f'c{k}_R': R[0], f'c{k}_t_start': KM.ARB_T_START,
                    f'c{k}_W0': W0, f'c{k}_W': W, f'c{k}_cost': cost, f'c{k}_feas': feas, f'c{k}_gmin': gmin, f'c{k}_nit': res.nit})
    out['n_cases'] = len(CASES)
    np.savez_compressed(os.path.join(HERE, 'nlp_keepout_moving_slsqp.npz'), **out)


if __name__ == '__main__':
    main()
