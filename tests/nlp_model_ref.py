"""CPU statement of the collocation solver under a quadratic objective model (include/d2d.h d2d_nlp_solve_model; test infrastructure
only).  It is oracle/nlp.py's algorithm on an oracle Problem whose structured cost terms are zero (kv = kphi = kobs = 0: what the
host-objective path hands the kernel), with the model

    m(W) = sum_i g_i . d_i + 1/2 d_i^T H_i d_i,   d_i = W_i - Wc_i

added in the three places that see the objective:

  merit / objective    + m(W)
  normal equations     the half gradient 1/2 (g_i + H_i d_i) on g and the half Hessian 1/2 H_i on the diagonal blocks (the solver's
                       convention: its g and D are halves)
  cost reported        m(W)

The solve loop is oracle.nlp.solve_general (through nlp_wind_ref.solve), which reaches these through the problem object.  H travels to the device as 15
planes, the upper triangle of each node's block row by row (include/d2d.h: plane a*5 - a*(a-1)/2 + (c-a) holds H[a][c], a <= c);
pack() / unpack() below state that order by enumeration, not by the formula.
"""
import numpy as np

import nlp_wind_ref as R
from oracle import nlp

NV, G_ACC = nlp.NV, nlp.G_ACC
PLANES = [(a, c) for a in range(NV) for c in range(a, NV)]         # (0,0) (0,1) .. (0,4) (1,1) .. (1,4) (2,2) .. (4,4)


def pack(H):
    """(N, 5, 5) symmetric blocks -> (15, N) planes."""
    return np.stack([H[:, a, c] for a, c in PLANES])


def unpack(planes):
    """(15, N) planes -> (N, 5, 5) symmetric blocks."""
    H = np.zeros((planes.shape[1], NV, NV))
    for k, (a, c) in enumerate(PLANES):
        H[:, a, c] = planes[k]; H[:, c, a] = planes[k]
    return H


class ModelProblem:
    """pb: an oracle Problem with kv = kphi = kobs = 0 (its constant wind and its bounds are used); g, Wc (N, 5); H (N, 5, 5)."""

    def __init__(self, pb, g, H, Wc):
        assert pb.kv == 0.0 and pb.kphi == 0.0 and pb.kobs == 0.0 and pb.kcol == 0.0
        self.pb, self.g, self.H, self.Wc = pb, np.asarray(g, float), np.asarray(H, float), np.asarray(Wc, float)
        assert np.array_equal(self.H, self.H.transpose(0, 2, 1))

    def value(self, W):
        d = W - self.Wc
        return float(np.sum(self.g * d) + 0.5 * np.einsum('ni,nij,nj->', d, self.H, d))

    def gradient(self, W):
        return self.g + np.einsum('nij,nj->ni', self.H, W - self.Wc)

    def constraints(self, W):
        return nlp.constraints(self.pb, W)

    def normal_equations(self, W, mu, rho):
        g, D, E = nlp._normal_equations(self.pb, W, mu, rho)
        return g + 0.5 * self.gradient(W), D + 0.5 * self.H, E

    def merit(self, W, mu, rho, mub, hasL, hasU):
        return nlp._merit(self.pb, W, mu, rho, mub, hasL, hasU) + self.value(W)

    def cost(self, W):
        return self.value(W)


def solve(mp, W0, **kw):
    return R.solve(mp, W0, **kw)


def kkt_residual(mp, W, mult, zL, zU):
    """oracle.nlp.kkt_residual with the model's gradient g + H d for cost_grad: stationarity of the Lagrangian with the bound duals,
    and feasibility."""
    pb = mp.pb
    h = pb.h
    x, y, psi, phi, v = W.T
    g = mp.gradient(W)
    sp, cp = np.sin(psi[1:]), np.cos(psi[1:]); tp = np.tan(phi[1:]); vi = v[1:]
    m = mult
    g[1:, 0] += m[:, 0] / h; g[:-1, 0] -= m[:, 0] / h
    g[1:, 1] += m[:, 1] / h; g[:-1, 1] -= m[:, 1] / h
    g[1:, 2] += m[:, 2] / h + m[:, 0] * vi * sp - m[:, 1] * vi * cp; g[:-1, 2] -= m[:, 2] / h
    g[1:, 3] += -m[:, 2] * G_ACC * (1 + tp * tp) / vi
    g[1:, 4] += -m[:, 0] * cp - m[:, 1] * sp + m[:, 2] * G_ACC * tp / (vi * vi)
    fixed = pb.lo == pb.hi
    return float(np.abs(np.where(fixed, 0.0, g - zL + zU)).max()), float(np.abs(nlp.constraints(pb, W)).max())
