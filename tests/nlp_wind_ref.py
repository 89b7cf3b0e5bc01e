"""CPU statement of the collocation solver in a wind field that varies in space and time (include/d2d.h d2d_nlp_solve_wind; test
infrastructure only).

It is oracle/nlp.py's algorithm -- augmented Lagrangian, primal-dual log barrier, damped Newton steps on the block-tridiagonal
Lagrangian Hessian -- with the three places that see the wind restated for a field F (a d2d.wind.SplineWindField, evaluated through
F.derivatives: the numpy twin of the kernel's wind_eval2):

  constraints        c_i = ... + F(t_i, x_i, y_i),  t_i = t_start + i h  (+ the field: the model's sign quirk)
  normal equations   with J = dF/d(x, y) at node i: the constraint Jacobian wrt its own node gains J on its (x, y) columns
                     (A[0][0] = 1/h + J00, A[0][1] = J01, A[1][0] = J10, A[1][1] = 1/h + J11), and the diagonal block the constraint
                     curvature rho (c + mu)_0 Hess(Fx) + rho (c + mu)_1 Hess(Fy) on (x, y).  Node i+1's constraint sees node i only
                     through -1/h: those terms do not change
  kkt_residual       the multipliers act on (x, y) of their own node through (I/h + J)^T

Everything that does not touch the wind is oracle/nlp.py's own code: the objective and its gradient, the banded solve, the barrier
sets, the constants -- and the solve loop, oracle.nlp.solve_general, which reaches the first two through the problem object
(FieldProblem below; tests/nlp_model_ref.py supplies another).  This statement supplies no family of node inequalities and no border.
"""
import numpy as np

from oracle import nlp

NV, G_ACC = nlp.NV, nlp.G_ACC


class FieldProblem:
    """An oracle Problem in a field: pb (its own wind is not used), the field and the time of node 0."""

    def __init__(self, pb, field, t_start=0.0):
        self.pb, self.field, self.t_start = pb, field, float(t_start)
        self.t = self.t_start + np.arange(pb.N) * pb.h

    def jet(self, W):
        """w (2, N), J (2, 2, N), H (2, 3, N) of the field at the nodes."""
        return self.field.derivatives(self.t, W[:, 0], W[:, 1])

    # what oracle.nlp.solve_general asks of a problem object: the places that see the wind (below), and the value it reports.  Another statement of
    # the same solver (tests/nlp_model_ref.py) is a class with these four methods and `pb`.
    def constraints(self, W):
        return constraints(self, W)

    def normal_equations(self, W, mu, rho):
        return _normal_equations(self, W, mu, rho)

    def merit(self, W, mu, rho, mub, hasL, hasU):
        return _merit(self, W, mu, rho, mub, hasL, hasU)

    def cost(self, W):
        return nlp.cost(self.pb, W)


def constraints(fp, W):
    """(N-1, 3): backward-Euler collocation residuals in the field."""
    pb = fp.pb
    x, y, psi, phi, v = W.T
    h = pb.h
    wx, wy = fp.field.sample_many(fp.t[1:], x[1:], y[1:])
    c1 = (x[1:] - x[:-1]) / h - v[1:] * np.cos(psi[1:]) + wx
    c2 = (y[1:] - y[:-1]) / h - v[1:] * np.sin(psi[1:]) + wy
    c3 = (psi[1:] - psi[:-1]) / h - G_ACC / v[1:] * np.tan(phi[1:])
    return np.stack([c1, c2, c3], 1)


def _al_value(fp, W, mu, rho):
    c = constraints(fp, W)
    return nlp.objective(fp.pb, W) + rho * float(np.sum((c + mu) ** 2))


def _normal_equations(fp, W, mu, rho):
    """oracle/nlp.py _normal_equations (second order) with the field's Jacobian in A and its Hessians in D."""
    pb = fp.pb
    N, h = pb.N, pb.h
    x, y, psi, phi, v = W.T
    D = np.zeros((N, NV, NV)); E = np.zeros((N - 1, NV, NV)); g = np.zeros((N, NV))
    D[:, 4, 4] += pb.s * pb.kv; g[:, 4] += pb.s * pb.kv * (v - pb.vsp)
    if pb.bank_max:
        im = int(np.argmax(np.abs(phi)))
        sb = pb.s * pb.N * pb.kphi
        D[im, 3, 3] += sb; g[im, 3] += sb * phi[im]
    else:
        D[:, 3, 3] += pb.s * pb.kphi; g[:, 3] += pb.s * pb.kphi * phi
    for w, e, dx, dy, k2, _f in nlp._obst_terms(pb, W, quirk=True):
        we = w * e
        g[:, 0] += -k2 * we * dx; g[:, 1] += -k2 * we * dy
        D[:, 0, 0] += k2 * k2 * we * dx * dx; D[:, 0, 1] += k2 * k2 * we * dx * dy
        D[:, 1, 0] += k2 * k2 * we * dx * dy; D[:, 1, 1] += k2 * k2 * we * dy * dy
    c = constraints(fp, W) + mu
    _, J, Hs = fp.jet(W)
    J, Hs = J[:, :, 1:], Hs[:, :, 1:]
    sp, cp = np.sin(psi[1:]), np.cos(psi[1:])
    tp = np.tan(phi[1:]); vi = v[1:]
    A = np.zeros((N - 1, 3, NV))
    A[:, 0, 0] = 1 / h + J[0, 0]; A[:, 0, 1] = J[0, 1]; A[:, 0, 2] = vi * sp; A[:, 0, 4] = -cp
    A[:, 1, 0] = J[1, 0]; A[:, 1, 1] = 1 / h + J[1, 1]; A[:, 1, 2] = -vi * cp; A[:, 1, 4] = -sp
    A[:, 2, 2] = 1 / h; A[:, 2, 3] = -G_ACC * (1 + tp * tp) / vi; A[:, 2, 4] = G_ACC * tp / (vi * vi)
    D[1:] += rho * np.einsum('nki,nkj->nij', A, A)
    g[1:] += rho * np.einsum('nki,nk->ni', A, c)
    idx = np.arange(3)
    D[:-1, idx, idx] += rho / (h * h)
    g[:-1, :3] += -rho * c / h
    E[:, :, :3] += -rho * A.transpose(0, 2, 1) / h
    m = rho * c
    sec2 = 1 + tp * tp
    D[1:, 2, 2] += m[:, 0] * vi * cp + m[:, 1] * vi * sp
    D[1:, 2, 4] += m[:, 0] * sp - m[:, 1] * cp; D[1:, 4, 2] += m[:, 0] * sp - m[:, 1] * cp
    D[1:, 3, 3] += -m[:, 2] * 2 * G_ACC * tp * sec2 / vi
    D[1:, 3, 4] += m[:, 2] * G_ACC * sec2 / (vi * vi); D[1:, 4, 3] += m[:, 2] * G_ACC * sec2 / (vi * vi)
    D[1:, 4, 4] += -m[:, 2] * 2 * G_ACC * tp / (vi ** 3)
    # the field's curvature: (xx, xy, yy) of each component
    D[1:, 0, 0] += m[:, 0] * Hs[0, 0] + m[:, 1] * Hs[1, 0]
    d01 = m[:, 0] * Hs[0, 1] + m[:, 1] * Hs[1, 1]
    D[1:, 0, 1] += d01; D[1:, 1, 0] += d01
    D[1:, 1, 1] += m[:, 0] * Hs[0, 2] + m[:, 1] * Hs[1, 2]
    return g, D, E


def _merit(fp, W, mu, rho, mub, hasL, hasU):
    pb = fp.pb
    sl = np.where(hasL, W - pb.lo, 1.0); su = np.where(hasU, pb.hi - W, 1.0)
    if (sl <= 0).any() or (su <= 0).any():
        return np.inf
    return _al_value(fp, W, mu, rho) - mub * float(np.sum(np.log(sl)) + np.sum(np.log(su)))


def solve(fp, W0, rho0=nlp.RHO0, inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX, feas_tol=nlp.FEAS_TOL, opt_tol=nlp.OPT_TOL):
    """oracle.nlp.solve_general in the field: no families, no border.  fp: a FieldProblem, or any object with `pb` and its four methods
    constraints, normal_equations, merit and cost.  Returns W, info (cost, feas, outer, inner, status, rho, mult, zL, zU, path)."""
    return nlp.solve_general(fp, W0, rho0=rho0, inner_max=inner_max, outer_max=outer_max, feas_tol=feas_tol, opt_tol=opt_tol)[:2]


def kkt_residual(fp, W, mult, zL=None, zU=None):
    """oracle.nlp.kkt_residual in the field: stationarity of cost_grad + A^T mult, and feasibility."""
    pb = fp.pb
    h = pb.h
    x, y, psi, phi, v = W.T
    g = nlp.cost_grad(pb, W)
    _, J, _ = fp.jet(W)
    J = J[:, :, 1:]
    sp, cp = np.sin(psi[1:]), np.cos(psi[1:]); tp = np.tan(phi[1:]); vi = v[1:]
    m = mult
    g[1:, 0] += m[:, 0] * (1 / h + J[0, 0]) + m[:, 1] * J[1, 0]; g[:-1, 0] -= m[:, 0] / h
    g[1:, 1] += m[:, 0] * J[0, 1] + m[:, 1] * (1 / h + J[1, 1]); g[:-1, 1] -= m[:, 1] / h
    g[1:, 2] += m[:, 2] / h + m[:, 0] * vi * sp - m[:, 1] * vi * cp; g[:-1, 2] -= m[:, 2] / h
    g[1:, 3] += -m[:, 2] * G_ACC * (1 + tp * tp) / vi
    g[1:, 4] += -m[:, 0] * cp - m[:, 1] * sp + m[:, 2] * G_ACC * tp / (vi * vi)
    feas = float(np.abs(constraints(fp, W)).max())
    if zL is not None:
        fixed = pb.lo == pb.hi
        return float(np.abs(np.where(fixed, 0.0, g - zL + zU)).max()), feas
    return float(np.abs(nlp._projected_gradient(pb, W, g)).max()), feas


def uniform_field(c, box=(-200.0, 200.0, -200.0, 200.0), h=50.0):
    """A spline field whose control points are all c = (cx, cy): spatially uniform (the weights of a B-spline sum to one)."""
    from d2d.wind import SplineWindField
    nx = int(round((box[1] - box[0]) / h)) + 3; ny = int(round((box[3] - box[2]) / h)) + 3
    cp = np.zeros((2, ny, nx)); cp[0] = c[0]; cp[1] = c[1]
    return SplineWindField(cp, box[0], h, box[2], h)


# ---- the problems of tests/test_gpu_nlp_wind.py (chosen on the CPU: this statement converges on every one of them) ----------------
T_GRID = np.arange(0.0, 14.5, 1.0)              # sample times of the unsteady field (covers 12 s horizons with margin)


def fields():
    """name -> SplineWindField in the style of tests/wind_ref.py: |w| <= 5 m/s, gradients <= 0.2 /s; the gust is unsteady.  The box
    (-150 .. 150, -200 .. 150) holds every pose of field_problems with margin."""
    import wind_ref as WR
    return {'shear': WR.spline_of(WR.shear), 'vortex': WR.spline_of(WR.vortex), 'gust': WR.spline_of(WR.gust, t=T_GRID)}


def field_problems(N, seed):
    """A ragged batch of oracle Problems with N nodes (h = 0.1) and their 'tri' guesses: 41 nodes -- four legs like those of
    tests/test_gpu_nlp.py's batch (46 m in 4 s); 121 nodes -- three perturbed exp_14 legs (12 s; ended 30 m short of exp_14's, so that
    5 m/s against the leg leave room below v_max); an obstacle on every second row.
    Chosen on the CPU, by this statement alone: it converges on every problem in every field of fields() (KKT residual <= 3e-6), and
    its Newton-step count is DETERMINED -- it moves by at most 2 when the guess moves by 1e-9.  The 121-node legs have obj_scale = N
    for that (cost of order 1 .. 100, as in test_ragged_node_counts_vs_oracle): with obj_scale = 1 their cost is 0.03 .. 3, the
    minimiser is flat and the statement's own step count moved by up to 140 under that perturbation (210 -> 289, 422 -> 282), so a
    comparison of step counts to +-10 would compare rounding.  A fourth 121-node leg was left out: in the gust the statement itself
    does not settle on it (240 against 101 steps under the perturbation, KKT residual 2e-2)."""
    from oracle import costs as C
    rng = np.random.default_rng(seed)
    h = 0.1
    pbs, W0s, obs = [], [], []
    for i in range(4 if N == 41 else 3):
        if N == 41:
            p0 = (0., 0., rng.uniform(-0.5, 0.5), 0., 12.); p1 = (46. + rng.uniform(-3, 3), rng.uniform(-6, 6), rng.uniform(-0.4, 0.4), 0., 12.)
            ob = [(23. + rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 6))] if i % 2 else []
            kw = dict(kv=5., kphi=1., obj_scale=1.0, phi_max=np.deg2rad(35.), v_min=9., v_max=15.)
        else:
            p0 = (-49.98 + rng.uniform(-5, 5), -58.14 + rng.uniform(-5, 5), 2.22 + rng.uniform(-0.2, 0.2), 0., 12.)
            p1 = (45. + rng.uniform(-5, 5), 20. + rng.uniform(-5, 5), rng.uniform(-0.2, 0.2), 0., 12.)
            ob = [(10. + rng.uniform(-5, 5), -10. + rng.uniform(-5, 5), rng.uniform(6, 10))] if i % 2 else []
            kw = dict(kv=1., kphi=0.5, obj_scale=float(N), phi_max=np.deg2rad(40.), v_min=9., v_max=15., x_box=(-150, 150), y_box=(-150, 150))
        pb = nlp.Problem(N, h, p0, p1, vsp=12., obstacles=ob, kobs=1.0 if ob else 0.0, obs_kind=1, **kw)
        pbs.append(pb); obs.append(ob)
        W0s.append(nlp.from_free(C.single_guess('tri', p0, p1, 12., (N - 1) * h, N), N))
    return pbs, W0s, obs
