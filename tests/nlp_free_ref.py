"""CPU statement of the collocation solver with a FREE time step (include/d2d.h d2d_nlp_solve_free; test infrastructure only).

It is oracle/nlp.py's algorithm -- augmented Lagrangian, primal-dual log barrier, damped Newton steps on the block-tridiagonal
Lagrangian Hessian -- with one more unknown: the node interval h, shared by every collocation equality.  The solver's variable is
u = 1 / h, in which every equality is LINEAR,  c_i = (s_i - s_{i-1}) u - f(s_i):  with D_i = (x, y, psi)_i - (x, y, psi)_{i-1}

  dc_i/du = D_i,   d2c_i/du2 = 0,   d2c_i/(du dw) = +1 on (x, y, psi)_i and -1 on (x, y, psi)_{i-1}

  objective      the row's structured cost + k_dur (N - 1) / u            (the duration, k_dur >= 0)
  box            1 / h_hi < u < 1 / h_lo, on the same log barrier as the node variables, with two duals of its own
  Newton system  [A b; b^T d] (dW, du) = (r, r_u) / 2:  A the block-tridiagonal matrix of oracle.nlp (at h = 1 / u),
                 b = rho J^T D + rho (c + mu) d2c/(du dw)      (half convention, like A)
                 d = k_dur (N - 1) / u^3 + rho |D|^2 + the barrier diagonal of u, damped like A's diagonal: d += lam max(|d|, 1e-12)
                 solved by the Schur complement on d:  x0 = A^-1 r / 2,  y = A^-1 b,  du = (r_u / 2 - b.x0) / (d - b.y),  dW = x0 - y du;
                 d - b.y <= 0: the bordered matrix is not positive definite -- the damping is raised as for a failed pivot

Everything that does not see h is oracle/nlp.py's own code, called at a copy of the Problem with h = 1 / u -- the solve loop too:
oracle.nlp.solve_general, to which this file supplies the border (Border: u, its box, its two duals, bordered_solve) and a problem
object whose methods take u (FreeProblem).  The interface speaks h: solve() takes the start interval and returns the solved one.
"""
import copy
import functools

import numpy as np

from oracle import nlp

NV, G_ACC = nlp.NV, nlp.G_ACC


class FreeProblem:
    """An oracle Problem whose interval is free in (h_lo, h_hi); pb.h is not used.  k_dur: weight of the duration (N - 1) h."""

    def __init__(self, pb, h_lo, h_hi, k_dur=0.0):
        self.pb, self.h_lo, self.h_hi, self.k_dur = pb, float(h_lo), float(h_hi), float(k_dur)
        self.u_lo, self.u_hi = 1.0 / self.h_hi, 1.0 / self.h_lo

    def at(self, u):
        p = copy.copy(self.pb)
        p.h = 1.0 / u
        return p

    def constraints(self, W, u):
        return nlp.constraints(self.at(u), W)

    def duration_cost(self, u):
        return self.k_dur * (self.pb.N - 1) / u

    def cost(self, W, u):
        """the reference's cost() + k_dur (N - 1) h"""
        return nlp.cost(self.pb, W) + self.duration_cost(u)

    def merit(self, W, u, mu, rho, mub, hasL, hasU):
        if not (self.u_lo < u < self.u_hi):
            return np.inf
        m = nlp._merit(self.at(u), W, mu, rho, mub, hasL, hasU)
        return m + self.duration_cost(u) - mub * (np.log(u - self.u_lo) + np.log(self.u_hi - u))

    def normal_equations(self, W, u, mu, rho):
        """g, D, E of oracle.nlp at h = 1 / u, and the u row: half gradient g_u, border b (N, 5), half curvature d_u."""
        pb = self.at(u)
        g, D, E = nlp._normal_equations(pb, W, mu, rho)
        N = pb.N
        x, y, psi, phi, v = W.T
        c = nlp.constraints(pb, W) + mu
        dl = W[1:, :3] - W[:-1, :3]
        sp, cp = np.sin(psi[1:]), np.cos(psi[1:]); tp = np.tan(phi[1:]); vi = v[1:]
        A = np.zeros((N - 1, 3, NV))
        A[:, 0, 0] = u; A[:, 0, 2] = vi * sp; A[:, 0, 4] = -cp
        A[:, 1, 1] = u; A[:, 1, 2] = -vi * cp; A[:, 1, 4] = -sp
        A[:, 2, 2] = u; A[:, 2, 3] = -G_ACC * (1 + tp * tp) / vi; A[:, 2, 4] = G_ACC * tp / (vi * vi)
        b = np.zeros((N, NV))
        b[1:] += rho * np.einsum('nki,nk->ni', A, dl)
        b[1:, :3] += rho * c                                  # cross curvature: +1 on the node's own (x, y, psi)
        b[:-1, :3] += -rho * u * dl - rho * c                 # the next node's equality: Jacobian -u, cross curvature -1
        kd = self.k_dur * (N - 1)
        g_u = -0.5 * kd / (u * u) + rho * float(np.sum(c * dl))
        d_u = kd / (u ** 3) + rho * float(np.sum(dl * dl))
        return g, D, E, g_u, b, d_u


def bordered_solve(Dh, E, rhs_half, free, lam, b, d, ru_half):
    """[A b; b^T d] (dw, du) = (rhs_half, ru_half) on the free variables by the Schur complement on d (d: damped already).
    Raises LinAlgError when A or the complement is not positive."""
    x0 = nlp._solve_block_tridiag(Dh, E, rhs_half, free, lam)
    yb = nlp._solve_block_tridiag(Dh, E, b, free, lam)
    bf = np.where(free, b, 0.0)
    sc = d - float(np.sum(bf * yb))
    if not sc > 0.0:
        raise np.linalg.LinAlgError('border')
    du = (ru_half - float(np.sum(bf * x0))) / sc
    return x0 - yb * du, du


class Border:
    """The bordered unknown oracle.nlp.solve_general asks for: u = 1 / h strictly inside (u_lo, u_hi), with the duals zl, zu of its
    two bounds on the same log barrier as the node variables."""
    solve = staticmethod(bordered_solve)

    def __init__(self, fp, h_start):
        self.lo, self.hi = fp.u_lo, fp.u_hi
        u = 1.0 / float(h_start)
        ku = min(1e-2 * max(1.0, abs(u)), 1e-2 * (self.hi - self.lo))
        self.u = min(max(u, self.lo + ku), self.hi - ku)

    def start_duals(self, mub):
        self.zl, self.zu = mub / (self.u - self.lo), mub / (self.hi - self.u)

    def kkt_error(self, g_u, mub):
        """stationarity of the u row and the complementarity of its two bounds"""
        sl, su = self.u - self.lo, self.hi - self.u
        return abs(2.0 * g_u - self.zl + self.zu), abs(self.zl * sl - mub), abs(self.zu * su - mub)

    def row(self, g_u, d_u, mub):
        """r_u, the right-hand side of the u row (full convention), and d0, its half curvature with the barrier diagonal (undamped)"""
        sl, su = self.u - self.lo, self.hi - self.u
        return -(2.0 * g_u - mub / sl + mub / su), d_u + 0.5 * (self.zl / sl + self.zu / su)

    def ratio(self, du, tau):
        """fraction to the boundary of u for the step du"""
        if du < 0:
            return -tau * (self.u - self.lo) / du
        if du > 0:
            return tau * (self.hi - self.u) / du
        return np.inf

    def dual_step(self, du, mub, tau):
        """the steps of the two duals and their ratio test"""
        sl, su = self.u - self.lo, self.hi - self.u
        dzl = mub / sl - self.zl - self.zl / sl * du
        dzu = mub / su - self.zu + self.zu / su * du
        az = np.inf
        if dzl < 0:
            az = min(az, -tau * self.zl / dzl)
        if dzu < 0:
            az = min(az, -tau * self.zu / dzu)
        return (dzl, dzu), az

    def accept(self, u, az, dz, mub):
        """the accepted step: the new u, and the duals stepped by az and clipped like the box duals"""
        self.u = u
        zl, zu = self.zl + az * dz[0], self.zu + az * dz[1]
        self.zl = float(np.clip(zl, mub / (1e10 * (u - self.lo)), 1e10 * mub / (u - self.lo)))
        self.zu = float(np.clip(zu, mub / (1e10 * (self.hi - u)), 1e10 * mub / (self.hi - u)))


def solve(fp, W0, h_start, rho0=nlp.RHO0, inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX, feas_tol=nlp.FEAS_TOL, opt_tol=nlp.OPT_TOL):
    """oracle.nlp.solve with the interval free.  Returns W, info (cost, feas, h, u, outer, inner, status, rho, mult, zL, zU, zu = the two
    duals of u, path).  mult = 2 rho mu is what the kernel returns: the estimate the last inner problem STARTED from; mult_last =
    2 rho (mu + c) is the one that problem is stationary with (what the next update would store): the multipliers of the KKT check."""
    bd = Border(fp, h_start)
    W, info, end = nlp.solve_general(fp, W0, border=bd, rho0=rho0, inner_max=inner_max, outer_max=outer_max, feas_tol=feas_tol,
                                     opt_tol=opt_tol)
    info.update(h=1.0 / bd.u, u=bd.u, zu=(bd.zl, bd.zu), mult_last=2 * info['rho'] * (end['mu'] + fp.constraints(W, bd.u)))
    return W, info


def kkt_residual(fp, W, h, mult, zL, zU, zu):
    """oracle.nlp.kkt_residual at h, and the row of u = 1 / h:  d/du [k_dur (N - 1) / u + mult . c] - zu_lower + zu_upper.
    -> largest stationarity residual (node rows and the u row), feasibility."""
    u = 1.0 / h
    stat, feas = nlp.kkt_residual(fp.at(u), W, mult, zL, zU)
    dl = W[1:, :3] - W[:-1, :3]
    su = -fp.k_dur * (fp.pb.N - 1) / (u * u) + float(np.sum(mult * dl)) - zu[0] + zu[1]
    return max(stat, abs(su)), feas


# ---- the problems of tests/test_nlp_free_cpu.py and tests/test_gpu_nlp_free.py ---------------------------------------------------
H0 = 0.1


def free_rows(fps, h_start=0.0):
    """[B][4] = (h_lo, h_hi, k_dur, h_start) of FreeProblems."""
    return np.array([(fp.h_lo, fp.h_hi, fp.k_dur, h_start) for fp in fps])


def leg_problem(N, seed, k_dur=0.5, obstacle=None, box=False, h_box=(0.5, 2.0), wind=(0.0, 0.0), speed=11.5, obj_scale=None):
    """A leg of N nodes that `speed` m/s over the ground covers in (N - 1) H0 seconds, end poses drawn from `seed`; obstacle: None,
    1 or 0 (a disc of that kind beside the middle of the leg); box: a y box 1 % of the leg wider than the end poses.  The interval is
    free in H0 * h_box.  -> FreeProblem, scenario row, the bowed start of nlp_steps_ref._start."""
    import nlp_steps_ref as S
    L = speed * H0 * (N - 1)
    rng = np.random.default_rng([N, seed])
    p0 = (0.0, 0.0, rng.uniform(-0.3, 0.3)); p1 = (L * rng.uniform(0.93, 1.0), 0.12 * L * rng.uniform(-1, 1), rng.uniform(-0.3, 0.3))
    kw = dict(vsp=12.0, kv=5.0, kphi=1.0, obj_scale=(10.0 * N if N <= 5 else float(N) / 4) if obj_scale is None else obj_scale,
              phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0, wind=wind)
    ob, kind = [], 1
    if obstacle == 1:
        ob = [(0.5 * p1[0] + 0.02 * L, 0.5 * p1[1] - 0.03 * L, max(0.12 * L, 0.5))]
    if obstacle == 0:
        ob, kind = [(0.5 * p1[0] + 0.02 * L, 0.5 * p1[1] + 0.08 * L, max(0.1 * L, 3.2))], 0
    if box:
        kw.update(y_box=(min(0.0, p1[1]) - 0.01 * L, max(0.0, p1[1]) + 0.01 * L))
    kobs = 0.0 if not ob else 20.0 if (N <= 5 and kind == 1) else 1.0
    pb = nlp.Problem(N, H0, p0, p1, obstacles=ob, kobs=kobs, obs_kind=kind, **kw)
    r = S.scenario_row(pb, ob, kobs, 1 if (ob and kind == 0) else 0)
    W0 = S._start(p0, p1, N, int(rng.integers(1 << 30)))
    return FreeProblem(pb, H0 * h_box[0], H0 * h_box[1], k_dur), r, W0


def ext(W, info):
    """The iterate with its interval: W (N, 5) and the row (h, u, 0, 0, 0) under it -- what the step-by-step comparison measures."""
    return np.concatenate([W, [[info['h'], info['u'], 0.0, 0.0, 0.0]]])


def steps_case(cid, fp, W0, h_start=H0):
    """A nlp_steps_ref Case of one free solve: the iterate is ext(W, info); the start's last row is a place holder (not perturbed
    meaningfully: the solve reads h_start)."""
    import nlp_steps_ref as S

    def run(W0s, inner_max, outer_max):
        W, info = solve(fp, W0s[0][:-1], h_start, inner_max=inner_max, outer_max=outer_max)
        return ext(W, info)[None], dict(inner=(info['inner'],), status=(info['status'],), path=tuple(info['path']), raw=info)
    return S.Case(cid, np.concatenate([W0, np.zeros((1, 5))])[None], run,
                  lambda W, h: (fp.cost(W, 1.0 / h), float(np.abs(fp.constraints(W, 1.0 / h)).max())))


STEP_N = (3, 5, 17, 64, 65, 121, 122, 129)
STEP_TAGS = ('disc1', 'disc0', 'box')
# seed of a case: the first one, counted from 0, at which the statement is determined and keeps stepping after every budget
# (nlp_steps_ref.check; found on the CPU with the statement alone).  Not listed: 0.  The 3-node disc and box cases have no such seed
# among the first twelve: with one free node the statement solves the first inner problem within 8 steps at every one of them, so
# their budget (8, 1) ends on the convergence test (tests/test_nlp_free_cpu.py says which checks they are held to).
STEP_SEEDS = {(5, 'disc1'): 1, (64, 'disc1'): 1, (64, 'disc0'): 4, (64, 'box'): 1, (65, 'disc0'): 5, (121, 'disc1'): 1, (121, 'disc0'): 6, (121, 'box'): 2,
              (122, 'disc1'): 4, (122, 'disc0'): 14, (122, 'box'): 1, (129, 'disc1'): 9, (129, 'disc0'): 8, (129, 'box'): 3}


@functools.lru_cache(maxsize=None)
def steps_launch(N):
    """d2d_nlp_solve_free, one ragged launch of N nodes: a kind-1 disc with k_dur = 0.5, a kind-0 disc with k_dur = 0, constant wind
    with a y box and k_dur = 2.  -> cases, rows, free_rows, bounds (None)."""
    cases, rows, fps = [], [], []
    for tag in STEP_TAGS:
        kw = dict(disc1=dict(obstacle=1, k_dur=0.5), disc0=dict(obstacle=0, k_dur=0.0), box=dict(box=True, k_dur=2.0, wind=(1.0, -0.5)))[tag]
        fp, r, W0 = leg_problem(N, 100 * STEP_TAGS.index(tag) + STEP_SEEDS.get((N, tag), 0), **kw)
        cases.append(steps_case(f'free-{N}-{tag}', fp, W0)); rows.append(r); fps.append(fp)
    return cases, np.stack(rows), free_rows(fps), None


BOUNDS_41 = (-np.deg2rad(5.0), np.deg2rad(35.0), -0.2, 2.0)


@functools.lru_cache(maxsize=None)
def bounds_launch():
    """41 nodes, a left turn: d2d_nlp_opts.bounds (phi in [-5, +35] deg, psi in [-0.2, 2.0]) beside the same row without an override;
    and the same turn with h_lo 5 % above the interval of its own interior optimum, so that h ends on its lower bound."""
    import nlp_steps_ref as S
    from oracle import costs as C
    N = 41
    p0 = (0.0, 0.0, 0.0, 0.0, 12.0); p1 = (26.0, 32.0, 1.8, 0.0, 12.0)
    mk = lambda: nlp.Problem(N, H0, p0, p1, vsp=12.0, kv=1.0, kphi=0.5, obj_scale=1.0, phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0)  # noqa: E731
    pa, pb = mk(), mk()
    pa.lo[:, 3], pa.hi[:, 3] = BOUNDS_41[0], BOUNDS_41[1]
    pa.lo[1:-1, 2], pa.hi[1:-1, 2] = BOUNDS_41[2], BOUNDS_41[3]
    W0 = nlp.from_free(C.single_guess('tri', p0, p1, 12.0, (N - 1) * H0, N), N)
    fa, fb = FreeProblem(pa, 0.05, 0.2, 1.0), FreeProblem(pb, 0.05, 0.2, 1.0)
    _, info = solve(fb, W0, H0)
    assert info['status'] == 1 and 0.05 * 1.06 < info['h'] < 0.19
    fc = FreeProblem(pb, 1.05 * info['h'], 0.2, 1.0)
    h_start = 1.3 * info['h']
    cases = [steps_case('free-bounds-interval', fa, W0), steps_case('free-bounds-row', fb, W0), steps_case('free-bounds-hlo', fc, W0, h_start)]
    fr = free_rows([fa, fb, fc]); fr[2, 3] = h_start
    r = S.scenario_row(pb)
    return cases, np.stack([r, r, r]), fr, np.array([BOUNDS_41, (0.0,) * 4, (0.0,) * 4])
