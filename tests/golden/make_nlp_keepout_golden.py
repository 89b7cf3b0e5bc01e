"""Generator of tests/golden/nlp_keepout_slsqp.npz: an arbiter of the collocation solve with hard keep-out discs that shares nothing with
the solver (csrc/nlp_kernels.hip d2d_nlp_solve_keepout) or the loop of its CPU statement (tests/nlp_keepout_ref.py) but the problem and
the start.

scipy's SLSQP minimises, over the free node values,

    objective(W)   subject to   the backward-Euler equalities,   the boxes,   |p_i - c_m|^2 - R_m^2 >= 0 at every interior node

with the node inequalities as TRUE constraints (type 'ineq', analytic Jacobians), ftol 1e-13.  The feasible set is not convex, so the
arbiter starts where the solver starts: the statement's start rule applied to the same W0 (nlp_keepout_ref.start) -- the side of the
disc a plan passes on is decided there, for both.  Cases: 5, 9 and 17 nodes; one disc whose centre is 0.3 R off the leg's axis; the same
disc and a second one that closes the near side.  Stored per case: the scenario row, the discs, W0, and SLSQP's cost (the reference's
cost()), feasibility, smallest g, iteration count and W.

Run from the repository root:  python tests/golden/make_nlp_keepout_golden.py
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'drone-sim-python_amd')]

import nlp_keepout_ref as K       # noqa: E402  (the problems and the start rule only)
from oracle import nlp            # noqa: E402

CASES = tuple((N, two) for N in K.ARB_N for two in (False, True))


def slsqp(pb, W0, discs):
    N = pb.N
    fixed, hasL, hasU = nlp._barrier_sets(pb)
    free = ~fixed
    Wf = np.where(fixed, pb.lo, W0)
    Wf = np.where(hasL, np.maximum(Wf, pb.lo + 1e-2 * (pb.hi - pb.lo)), Wf)
    Wf = np.where(hasU, np.minimum(Wf, pb.hi - 1e-2 * (pb.hi - pb.lo)), Wf)
    Wf = K.start(pb, Wf, discs)
    lo, hi = pb.lo[free], pb.hi[free]
    pos = np.cumsum(free.reshape(-1)).reshape(free.shape) - 1          # index of a free variable in z

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
        W = unpack(z)
        return K.g_values(W[1:-1], discs)[0].reshape(-1)

    def gjac(z):
        W = unpack(z)
        _, dx, dy = K.g_values(W[1:-1], discs)
        J = np.zeros((len(discs), N - 2, len(z)))
        for m in range(len(discs)):
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
    for k, (N, two) in enumerate(CASES):
        pb, row, W0, discs = K.arbiter_problem(N, two)
        W, res = slsqp(pb, W0, discs)
        cost, feas = nlp.cost(pb, W), float(np.abs(nlp.constraints(pb, W)).max())
        gmin = float((K.g_values(W[1:-1], discs)[0] / discs[:, 2:3] ** 2).min())
        print(f'case {k}: N {N}, {len(discs)} disc(s): {res.message!r} after {res.nit} iterations, cost {cost:.12f}, feas {feas:.2e}, min g / R^2 {gmin:.2e}')
        assert res.success and feas <= 1e-9 and gmin >= -1e-9
        out.update({f'c{k}_N': N, f'c{k}_row': row, f'c{k}_discs': discs, f'c{k}_W0': W0, f'c{k}_W': W, f'c{k}_cost': cost, f'c{k}_feas': feas,
                    f'c{k}_gmin': gmin, f'c{k}_nit': res.nit})
    out['n_cases'] = len(CASES)
    np.savez_compressed(os.path.join(HERE, 'nlp_keepout_slsqp.npz'), **out)


if __name__ == '__main__':
    main()
