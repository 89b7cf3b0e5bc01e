"""Generator of tests/golden/nlp_free_fence_slsqp.npz: an arbiter of the free-time-step collocation solve outside hard discs and inside a
convex polygon that shares nothing with the solver (csrc/nlp_kernels.hip d2d_nlp_solve_free_fence) or its CPU statement
(tests/nlp_free_fence_ref.py) but the problem.

scipy's SLSQP minimises, over the free node values and the interval h itself (NOT u = 1 / h),

    objective(W) + k_dur (N - 1) h    subject to   the backward-Euler equalities in the reference's form at h,   the boxes, h_lo <= h <= h_hi,
                                                   |p_i - c_m|^2 - R_m^2 >= 0   and   b_k - a_k . p_i >= 0   at every interior node

with analytic gradients (oracle.nlp.cost_grad; the Jacobians of the equalities and of the two families of inequalities written out
below), ftol 1e-12, from the same start as the solver moved out of the discs and into the polygon by hand (a radial push and a clip:
not the solver's start rule).  The end conditions are not variables.  Cases (nlp_free_fence_ref.ARB_CASES): 5, 9 and 17 nodes, k_dur > 0
so that h is determined; each is built so that a disc or an edge is ACTIVE at SLSQP's optimum (asserted: an inequality within 1e-7 of
zero), and h ends strictly inside its box.  Stored per case: the scenario row, the row of the step's box, the tables, the start, and
SLSQP's cost, h, feasibility, smallest inequality, iteration count and W.

Run from the repository root:  python tests/golden/make_nlp_free_fence_golden.py
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'drone-sim-python_amd')]

import nlp_free_fence_ref as FF   # noqa: E402  (the problems only: arbiter_problem)
from oracle import nlp            # noqa: E402


def slsqp(fp, W0, h_start, discs, edges):
    pb = fp.pb
    N = pb.N
    fixed = pb.lo == pb.hi
    free = ~fixed
    Wf = np.where(fixed, pb.lo, W0)
    lo, hi = pb.lo[free], pb.hi[free]
    kd = fp.k_dur * (N - 1)
    idx = -np.ones((N, 5), int)
    idx[free] = np.arange(int(free.sum()))
    nz = int(free.sum()) + 1

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

    def ineq(z):
        W, _ = unpack(z)
        p = W[1:-1, :2]
        gd = [(p[:, 0] - cx) ** 2 + (p[:, 1] - cy) ** 2 - R * R for cx, cy, R in discs]
        ge = [b - (ax * p[:, 0] + ay * p[:, 1]) for ax, ay, b, _ in edges]
        return np.concatenate(gd + ge) if gd or ge else np.zeros(0)

    def ineq_jac(z):
        W, _ = unpack(z)
        rows = []
        for cx, cy, R in discs:
            for i in range(1, N - 1):
                r = np.zeros(nz)
                r[idx[i, 0]] = 2.0 * (W[i, 0] - cx); r[idx[i, 1]] = 2.0 * (W[i, 1] - cy)
                rows.append(r)
        for ax, ay, b, _ in edges:
            for i in range(1, N - 1):
                r = np.zeros(nz)
                r[idx[i, 0]] = -ax; r[idx[i, 1]] = -ay
                rows.append(r)
        return np.array(rows).reshape(-1, nz)

    # the start, by hand: out of the discs radially (1.05 R), then inside the edges (1e-3 of the leg off each), then inside the boxes
    Ws = Wf.copy()
    for cx, cy, R in discs:
        d = Ws[1:-1, :2] - (cx, cy)
        dn = np.hypot(d[:, 0], d[:, 1])
        inside = dn < 1.05 * R
        Ws[1:-1, :2][inside] = (cx, cy) + d[inside] / dn[inside, None] * 1.05 * R
    ll = float(np.hypot(*(np.asarray(pb.p1[:2]) - np.asarray(pb.p0[:2]))))
    for ax, ay, b, _ in edges:
        g = b - (ax * Ws[1:-1, 0] + ay * Ws[1:-1, 1])
        t = np.maximum(1e-3 * ll - g, 0.0)
        Ws[1:-1, 0] -= t * ax; Ws[1:-1, 1] -= t * ay
    wd = np.where(np.isfinite(hi - lo), hi - lo, 1.0)
    z0 = np.concatenate([np.clip(Ws[free], lo + 1e-3 * wd, hi - 1e-3 * wd), [h_start]])
    bounds = [(a if np.isfinite(a) else None, b if np.isfinite(b) else None) for a, b in zip(lo, hi)] + [(fp.h_lo, fp.h_hi)]
    res = minimize(fun, z0, jac=grad, bounds=bounds, method='SLSQP', options=dict(ftol=1e-12, maxiter=800),
                   constraints=[dict(type='eq', fun=con, jac=jac), dict(type='ineq', fun=ineq, jac=ineq_jac)])
    W, h = unpack(res.x)
    return W, h, res, float(ineq(res.x).min())


def main():
    out = {}
    for k, name in enumerate(FF.ARB_CASES):
        fp, row, W0, discs, edges = FF.arbiter_problem(name)
        W, h, res, gmin = slsqp(fp, W0, FF.H0, discs, edges)
        cost, feas = fp.cost(W, 1.0 / h), float(np.abs(fp.constraints(W, 1.0 / h)).max())
        print(f'case {k}: {name}: {res.message!r} after {res.nit} iterations, cost {cost:.12f}, h {h:.12f}, feas {feas:.2e}, smallest g {gmin:.2e}')
        assert res.success and feas <= 1e-9 and fp.h_lo < h < fp.h_hi
        assert -1e-9 <= gmin <= 1e-7, 'no disc or edge is active at the optimum'
        out.update({f'c{k}_name': name, f'c{k}_N': fp.pb.N, f'c{k}_row': row, f'c{k}_free_row': np.array([fp.h_lo, fp.h_hi, fp.k_dur, 0.0]),
                    f'c{k}_discs': discs, f'c{k}_edges': edges, f'c{k}_W0': W0, f'c{k}_W': W, f'c{k}_cost': cost, f'c{k}_h': h,
                    f'c{k}_feas': feas, f'c{k}_gmin': gmin, f'c{k}_nit': res.nit})
    out['n_cases'] = len(FF.ARB_CASES)
    np.savez_compressed(os.path.join(HERE, 'nlp_free_fence_slsqp.npz'), **out)


if __name__ == '__main__':
    main()
