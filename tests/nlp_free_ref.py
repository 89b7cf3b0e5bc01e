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

Everything that does not see h is oracle/nlp.py's own code, called at a copy of the Problem with h = 1 / u.  The interface speaks h:
solve() takes the start interval and returns the solved one.
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


def solve(fp, W0, h_start, rho0=nlp.RHO0, inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX, feas_tol=nlp.FEAS_TOL, opt_tol=nlp.OPT_TOL):
    """oracle.nlp.solve with the interval free.  Returns W, info (cost, feas, h, u, outer, inner, status, rho, mult, zL, zU, zu = the two
    duals of u, path).  mult = 2 rho mu is what the kernel returns: the estimate the last inner problem STARTED from; mult_last =
    2 rho (mu + c) is the one that problem is stationary with (what the next update would store): the multipliers of the KKT check."""
    pb = fp.pb
    fixed, hasL, hasU = nlp._barrier_sets(pb)
    free = ~fixed
    W = np.asarray(W0, float).copy()
    W[fixed] = pb.lo[fixed]
    width = np.where(hasL & hasU, pb.hi - pb.lo, np.inf)
    kap = np.minimum(1e-2 * np.maximum(1.0, np.abs(W)), 1e-2 * width)
    W = np.where(hasL, np.maximum(W, pb.lo + kap), W)
    W = np.where(hasU, np.minimum(W, pb.hi - kap), W)
    u = 1.0 / float(h_start)
    ku = min(1e-2 * max(1.0, abs(u)), 1e-2 * (fp.u_hi - fp.u_lo))
    u = min(max(u, fp.u_lo + ku), fp.u_hi - ku)
    mu = np.zeros((pb.N - 1, 3)); rho = rho0
    mub = nlp.MUB0
    zL = np.where(hasL, mub / np.where(hasL, W - pb.lo, 1.0), 0.0)
    zU = np.where(hasU, mub / np.where(hasU, pb.hi - W, 1.0), 0.0)
    zul, zuu = mub / (u - fp.u_lo), mub / (fp.u_hi - u)
    lam = nlp.LAM0
    feas_prev = np.inf
    total_inner = 0
    status = 2
    n_stalled = 0
    path = []
    if pb.bank_max:
        inner_max, outer_max = nlp.BANKMAX_BATCHES * inner_max, (outer_max + nlp.BANKMAX_BATCHES - 1) // nlp.BANKMAX_BATCHES
    for outer in range(1, outer_max + 1):
        tol_in = max(opt_tol, min(1e-1, 10.0 * mub), nlp.GRAD_FLOOR * rho)
        phi_first = phi_last = None
        for it in range(inner_max):
            total_inner += 1
            sl = np.where(hasL, W - pb.lo, 1.0); su = np.where(hasU, pb.hi - W, 1.0)
            sul, suu = u - fp.u_lo, fp.u_hi - u
            g, D, E, g_u, b, d_u = fp.normal_equations(W, u, mu, rho)
            stat = np.where(free, 2.0 * g - zL + zU, 0.0)
            comp = max(float(np.abs(np.where(hasL, zL * sl - mub, 0.0)).max()), float(np.abs(np.where(hasU, zU * su - mub, 0.0)).max()))
            err = max(float(np.abs(stat).max()), comp, abs(2.0 * g_u - zul + zuu), abs(zul * sul - mub), abs(zuu * suu - mub))
            if err <= tol_in:
                break
            sig = np.where(hasL, zL / sl, 0.0) + np.where(hasU, zU / su, 0.0)
            rhs = -(2.0 * g - np.where(hasL, mub / sl, 0.0) + np.where(hasU, mub / su, 0.0))
            r_u = -(2.0 * g_u - mub / sul + mub / suu)
            Dh = D.copy()
            idx = np.arange(NV)
            Dh[:, idx, idx] += 0.5 * sig
            d0 = d_u + 0.5 * (zul / sul + zuu / suu)
            phi0 = fp.merit(W, u, mu, rho, mub, hasL, hasU)
            if phi_first is None:
                phi_first = phi_last = phi0
            accepted = False
            raised = 0
            for _ in range(30):
                try:
                    dw, du = bordered_solve(Dh, E, 0.5 * rhs, free, lam, b, d0 + lam * max(abs(d0), 1e-12), 0.5 * r_u)
                except np.linalg.LinAlgError:
                    lam = min(lam * 8.0, nlp.LAM_MAX); raised += 1; continue
                dphi = -(float(np.sum(rhs * dw)) + r_u * du)
                if not dphi < 0.0:
                    lam = min(lam * 8.0, nlp.LAM_MAX); raised += 1; continue
                tau = max(0.99, 1.0 - mub)
                with np.errstate(divide='ignore', invalid='ignore'):
                    aL = np.where(hasL & (dw < 0), -tau * sl / dw, np.inf)
                    aU = np.where(hasU & (dw > 0), tau * su / dw, np.inf)
                amax = min(1.0, float(aL.min()), float(aU.min()))
                if du < 0:
                    amax = min(amax, -tau * sul / du)
                if du > 0:
                    amax = min(amax, tau * suu / du)
                a = amax
                ok = False
                for _ls in range(8):
                    Wt, ut = W + a * dw, u + a * du
                    pt = fp.merit(Wt, ut, mu, rho, mub, hasL, hasU)
                    if np.isfinite(pt) and pt <= phi0 + 1e-4 * a * dphi:
                        ok = True
                        break
                    a *= 0.5
                if ok:
                    dzL = np.where(hasL, mub / sl - zL - zL / sl * dw, 0.0)
                    dzU = np.where(hasU, mub / su - zU + zU / su * dw, 0.0)
                    dzul = mub / sul - zul - zul / sul * du
                    dzuu = mub / suu - zuu + zuu / suu * du
                    with np.errstate(divide='ignore', invalid='ignore'):
                        azL = np.where(hasL & (dzL < 0), -tau * zL / dzL, np.inf)
                        azU = np.where(hasU & (dzU < 0), -tau * zU / dzU, np.inf)
                    az = min(1.0, float(azL.min()), float(azU.min()))
                    if dzul < 0:
                        az = min(az, -tau * zul / dzul)
                    if dzuu < 0:
                        az = min(az, -tau * zuu / dzuu)
                    path.append((a, max(float(np.abs(Wt - W).max()), abs(ut - u)), raised, _ls))
                    W, u = Wt, ut
                    phi_last = pt
                    zL = zL + az * dzL; zU = zU + az * dzU
                    zul, zuu = zul + az * dzul, zuu + az * dzuu
                    slp = np.where(hasL, W - pb.lo, 1.0); sup = np.where(hasU, pb.hi - W, 1.0)
                    zL = np.where(hasL, np.clip(zL, mub / (1e10 * slp), 1e10 * mub / slp), 0.0)
                    zU = np.where(hasU, np.clip(zU, mub / (1e10 * sup), 1e10 * mub / sup), 0.0)
                    zul = float(np.clip(zul, mub / (1e10 * (u - fp.u_lo)), 1e10 * mub / (u - fp.u_lo)))
                    zuu = float(np.clip(zuu, mub / (1e10 * (fp.u_hi - u)), 1e10 * mub / (fp.u_hi - u)))
                    lam = max(lam / 3.0, nlp.LAM_MIN) if a == amax else lam
                    accepted = True
                    break
                lam = min(lam * 4.0, nlp.LAM_MAX)
            if not accepted:
                break
        c = fp.constraints(W, u)
        feas = float(np.abs(c).max())
        if feas <= feas_tol and mub <= nlp.MUB_MIN * 1.0001 and err <= tol_in:
            status = 1
            break
        if pb.bank_max and feas <= feas_tol and mub <= nlp.MUB_MIN * 1.0001 and phi_first is not None \
                and (phi_first - phi_last) <= nlp.BANKMAX_VALUE_TOL * (1.0 + abs(phi_last)):
            status = 1
            break
        if err > tol_in and accepted and (phi_first - phi_last) > (nlp.BANKMAX_VALUE_TOL if pb.bank_max else nlp.GATE_PROGRESS) * (1.0 + abs(phi_last)):
            continue
        n_stalled = n_stalled + 1 if (feas > 0.5 * feas_prev and feas > 1e3 * feas_tol) else 0
        if n_stalled >= (3 if rho >= nlp.RHO_MAX else nlp.STALL_OUTERS):
            status = 4
            break
        mu = mu + c
        if feas > 0.25 * feas_prev and rho < nlp.RHO_MAX:
            mu = mu / nlp.RHO_GROW; rho *= nlp.RHO_GROW
        feas_prev = feas
        mub = max(nlp.MUB_MIN, min(0.2 * mub, mub ** 1.5))
    return W, dict(cost=fp.cost(W, u), feas=float(np.abs(fp.constraints(W, u)).max()), h=1.0 / u, u=u, outer=outer, inner=total_inner,
                   status=status, rho=rho, mult=2 * rho * mu, mult_last=2 * rho * (mu + fp.constraints(W, u)), zL=zL, zU=zU, zu=(zul, zuu),
                   path=path)


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
