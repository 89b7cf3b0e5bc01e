"""CPU statement of the collocation solver with HARD keep-out discs (include/d2d.h d2d_nlp_solve_keepout; test infrastructure only).

It is oracle/nlp.py's loop -- augmented Lagrangian, primal-dual log barrier, damped Newton steps on the block-tridiagonal Lagrangian
Hessian -- with one family of node inequalities: for every interior node i (x and y free: 1 .. N-2) and disc m = (cx, cy, R), R > 0,

    g_im = (x_i - cx)^2 + (y_i - cy)^2 - R^2 > 0,        d = (x_i - cx, y_i - cy),   s = the step of (x_i, y_i)

each with a dual z_im > 0 that is treated exactly like the box duals zL, zU:

  merit          - mub sum log g  (one log per node, of the product over the discs); +inf when any g <= 0
  stationarity   rows of (x_i, y_i):  ... - sum_m z 2d
  complementarity |z g - mub|, joined into err
  right-hand side the same rows with mub / g in the place of z
  Newton block   (x, y) corner of node i's diagonal block, half convention:  2 (z / g) d d^T - z I.  The - z I is the constraint's own,
                 negative, curvature; a matrix that is not positive definite raises lam eightfold (the banded Cholesky fails)
  dual step      dz = mub / g - z - (z / g) 2 d.s;  ratio test and clip to [mub / (1e10 g), 1e10 mub / g] as the box duals
  primal ratio   the largest a <= 1 with g + 2 a d.s + a^2 |s|^2 >= (1 - tau) g:  the smaller positive root (ratio_disc)
  start          after the box push, a free node with g <= kappa = (1.01^2 - 1) R^2 moves radially to |d| = 1.01 R (along the left normal
                 of the leg p0 -> p1 if |d| < 1e-12 R); discs in index order, two passes; then the box push again on x and y
  refusals       a non-finite disc, an end pose with g <= 0, a free node with g <= 0 after the start: status 3, NaN cost, W untouched

The loop is oracle.nlp.solve_general; this file supplies the family Discs, on per-node centres ctr (n, N, 2) and radii R (n,) -- a static
disc is a track that stands still (constant_centres) -- the start rule, the refusals and the scatter of the duals into zk (n, N).
tests/nlp_keepout_moving_ref.py and tests/nlp_fence_ref.py use the same family.  The problem object is solve_general's: Plain
(oracle.nlp's own functions, the rows' constant wind) or nlp_wind_ref.FieldProblem.  With no discs solve() is oracle.nlp.solve bit for bit.
"""
import functools

import numpy as np

from oracle import nlp
from oracle.nlp import Plain, _box_push      # noqa: F401  (tests and the other statements reach them as K.Plain, K._box_push)

NV = nlp.NV
ST_NONFINITE = 3
PUSH = 1e-2


def lowered_radius(r, margin, v_max, h):
    """R of the node constraint that keeps every point of the polyline `margin` from a disc of radius r: the chord between two nodes
    at spacing s <= v_max h that lie on the circle R passes the centre at sqrt(R^2 - (s/2)^2) >= r + margin."""
    return float(np.sqrt((r + margin) ** 2 + (0.5 * v_max * h) ** 2))


def constant_centres(discs, N):
    """The tables of static discs (n, 3) = (cx, cy, R) as tracks that stand still: ctr (n, N, 2), R (n,)."""
    discs = np.asarray(discs, float).reshape(-1, 3)
    return np.repeat(discs[:, None, :2], N, axis=1), discs[:, 2].copy()


def ratio_disc(g, bh, aa, tau):
    """Fraction to the boundary of one disc: the largest a with g + 2 a bh + a^2 aa >= (1 - tau) g on [0, a] (bh = d.s, aa = |s|^2;
    elementwise, inf where nothing binds): the smaller positive root of aa a^2 + 2 bh a + tau g, as tau g / (sqrt(disc) - bh)."""
    g, bh, aa = np.broadcast_arrays(np.asarray(g, float), np.asarray(bh, float), np.asarray(aa, float))
    cq = tau * g
    disc = bh * bh - aa * cq
    ok = (bh < 0.0) & (disc > 0.0)
    return np.where(ok, cq / (np.sqrt(np.where(ok, disc, 1.0)) - np.where(ok, bh, -1.0)), np.inf)


# ---- the discs on per-node centres: the one implementation (the finite-difference tests pin these through the adapters below) --------
def disc_g(W, ctr, R):
    """(n, M) g of every (disc, row of W) against ctr (n, M, 2) -- the rows' own centres -- and dx, dy (n, M)."""
    dx = W[None, :, 0] - ctr[:, :, 0]; dy = W[None, :, 1] - ctr[:, :, 1]
    return dx * dx + dy * dy - R[:, None] ** 2, dx, dy


def disc_barrier_value(W, ctr, R, mub):
    """- mub sum log g over the interior nodes (one log per node, of the product over the discs, as the kernel takes it); +inf when a
    g <= 0.  This is what the loop's merit adds for the discs."""
    gk = disc_g(W[1:-1], ctr[:, 1:-1], R)[0]
    if (gk <= 0.0).any():
        return np.inf
    return -mub * float(np.sum(np.log(np.prod(gk, axis=0))))


def disc_barrier_terms(W, ctr, R, zk, mub):
    """What the loop adds for the discs at (W, zk): rhs (N, 2) [full convention, the negative merit gradient with mub / g], the
    stationarity term (N, 2) and the half-convention 2x2 blocks (N, 2, 2)."""
    N = len(W)
    gk, dx, dy = disc_g(W[1:-1], ctr[:, 1:-1], R)
    mg, zg = mub / gk, zk / gk
    rhs = np.zeros((N, 2)); st = np.zeros((N, 2)); blk = np.zeros((N, 2, 2))
    rhs[1:-1, 0] = np.sum(2.0 * mg * dx, axis=0); rhs[1:-1, 1] = np.sum(2.0 * mg * dy, axis=0)
    st[1:-1, 0] = -np.sum(2.0 * zk * dx, axis=0); st[1:-1, 1] = -np.sum(2.0 * zk * dy, axis=0)
    blk[1:-1, 0, 0] = np.sum(2.0 * zg * dx * dx - zk, axis=0); blk[1:-1, 1, 1] = np.sum(2.0 * zg * dy * dy - zk, axis=0)
    blk[1:-1, 0, 1] = blk[1:-1, 1, 0] = np.sum(2.0 * zg * dx * dy, axis=0)
    return rhs, st, blk


def disc_rule(pb, W, ctr, R):
    """The discs' start rule, node i against its own centres: every interior node out of the discs (no box push)."""
    W = W.copy()
    leg = pb.p1[:2] - pb.p0[:2]; ll = float(np.sqrt(leg[0] * leg[0] + leg[1] * leg[1]))
    nrm = (-leg[1] / ll, leg[0] / ll) if ll > 0.0 else (0.0, 1.0)
    for i in range(1, pb.N - 1):
        x, y = W[i, 0], W[i, 1]
        for _pass in range(2):
            for m in range(len(R)):
                Rm = R[m]
                if not Rm > 0.0:
                    continue
                cx, cy = ctr[m, i]
                Rt = Rm * (1.0 + PUSH)
                dx, dy = x - cx, y - cy
                d2 = dx * dx + dy * dy
                if d2 - Rm * Rm <= Rt * Rt - Rm * Rm:
                    dn = np.sqrt(d2)
                    ux, uy = nrm if dn < 1e-12 * Rm else (dx / dn, dy / dn)
                    x, y = cx + Rt * ux, cy + Rt * uy
        W[i, 0], W[i, 1] = x, y
    return W


def push_xy(pb, W):
    """The box push on x and y alone, in place: what closes every start rule."""
    _, hasL, hasU = nlp._barrier_sets(pb)
    W[:, :2] = _box_push(W[:, :2], pb.lo[:, :2], pb.hi[:, :2], hasL[:, :2], hasU[:, :2])
    return W


def disc_start(pb, W, ctr, R):
    """The start rule on a W that has had the box push: disc_rule, then the box push again on x and y."""
    return push_xy(pb, disc_rule(pb, W, ctr, R))


def disc_refused(pb, ctr, R, W):
    """discs unusable for this problem (W: after disc_start())?  The end poses are held against their own nodes' centres."""
    if not (np.isfinite(R).all() and np.isfinite(ctr).all()):
        return True
    ia = np.flatnonzero(R > 0.0)
    if not len(ia):
        return False
    ends = np.array([pb.p0, pb.p1])
    if (disc_g(ends, ctr[ia][:, [0, -1]], R[ia])[0] <= 0.0).any():
        return True
    return bool((disc_g(W[1:-1], ctr[ia][:, 1:-1], R[ia])[0] <= 0.0).any())


class Discs:
    """The family of hard discs that oracle.nlp.solve_general asks for: the present ones (R > 0) of ctr (n, N, 2), R (n,)."""

    def __init__(self, ctr, R):
        self.n = len(R)
        self.ia = np.flatnonzero(R > 0.0)
        self.ctr, self.R = ctr[self.ia], R[self.ia]

    def __len__(self):
        return len(self.ia)

    def _at(self, W, dw=None):
        """g, and with a step dw: bh = d.s, aa = |s|^2 at the interior nodes"""
        gk, dx, dy = disc_g(W[1:-1], self.ctr[:, 1:-1], self.R)
        if dw is None:
            return gk
        sx, sy = dw[1:-1, 0], dw[1:-1, 1]
        return gk, dx * sx + dy * sy, sx * sx + sy * sy

    def g(self, W):
        return self._at(W)

    def barrier_value(self, W, mub):
        return disc_barrier_value(W, self.ctr, self.R, mub)

    def barrier_terms(self, W, z, mub):
        return disc_barrier_terms(W, self.ctr, self.R, z, mub)

    def ratio(self, W, dw, tau):
        return ratio_disc(*self._at(W, dw), tau)

    def dual_step(self, W, dw, z, mub):
        gk, bh, _ = self._at(W, dw)
        return (mub - 2.0 * z * bh) / gk - z

    def scatter(self, z, N):
        """the duals (n_present, N - 2) -> zk (n, N): 0 at the end nodes and for absent discs"""
        zfull = np.zeros((self.n, N))
        zfull[self.ia, 1:-1] = z
        return zfull


# ---- the static table (n, 3): thin adapters, under the names the tests and the SLSQP golden generators call -------------------------
def g_values(W, discs):
    """(n, N) g of every (disc, node), and dx, dy (n, N)."""
    return disc_g(W, *constant_centres(discs, len(W)))


def barrier_value(W, act, mub):
    return disc_barrier_value(W, *constant_centres(act, len(W)), mub)


def barrier_terms(W, act, zk, mub):
    return disc_barrier_terms(W, *constant_centres(act, len(W)), zk, mub)


def start(pb, W, discs):
    """The start rule on a W that has had the box push: every interior node out of the discs, then the box push again on x and y."""
    return disc_start(pb, W, *constant_centres(discs, pb.N))


def refused(pb, discs, W):
    """discs unusable for this problem (W: after start())?"""
    return disc_refused(pb, *constant_centres(discs, pb.N), W)


def solve_discs(prob, W0, ctr, R, **schedule):
    """oracle.nlp.solve_general outside the discs of centres ctr (n, N, 2) and node radii R (n,) (R <= 0: absent): the box push, the
    start rule, the refusal, the loop with the family Discs, the scatter of its duals.  solve() here and nlp_keepout_moving_ref.solve
    are this."""
    pb = prob.pb
    W = nlp.interior_start(pb, W0)
    if len(R):
        if np.isfinite(R).all() and np.isfinite(ctr).all():
            W = disc_start(pb, W, ctr, R)
        if disc_refused(pb, ctr, R, W):
            return np.asarray(W0, float).copy(), dict(cost=np.nan, feas=np.nan, outer=0, inner=0, status=ST_NONFINITE, path=[],
                                                      zk=np.zeros((len(R), pb.N)))
    fam = Discs(ctr, R)
    W, info, end = nlp.solve_general(prob, W, families=(fam,), started=True, **schedule)
    info.update(zk=fam.scatter(end['z'][0], pb.N), mub=end['mub'])
    return W, info


def solve(prob, W0, discs, rho0=nlp.RHO0, inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX, feas_tol=nlp.FEAS_TOL, opt_tol=nlp.OPT_TOL):
    """oracle.nlp.solve outside the discs (n, 3) = (cx, cy, R) (R <= 0: absent).  Returns W, info of oracle.nlp.solve plus zk (n, N): the
    discs' duals (0 at the end nodes and for absent discs) and mub.  A refused problem: W0 itself, status 3, NaN cost and feas."""
    return solve_discs(prob, W0, *constant_centres(discs, prob.pb.N), rho0=rho0, inner_max=inner_max, outer_max=outer_max,
                       feas_tol=feas_tol, opt_tol=opt_tol)


def polyline_clearance(xy, c, r):
    """smallest |p - c| - r over the polyline through xy (N, 2)"""
    a, b = xy[:-1], xy[1:]
    ab = b - a
    t = np.clip(np.sum((np.asarray(c) - a) * ab, 1) / np.maximum(np.sum(ab * ab, 1), 1e-300), 0.0, 1.0)
    p = a + t[:, None] * ab
    return float(np.sqrt(np.sum((p - np.asarray(c)) ** 2, 1)).min() - r)


# ---- the problems of tests/test_nlp_keepout_cpu.py and tests/test_gpu_nlp_keepout.py --------------------------------------------------
H0 = 0.1
MAX_KEEP = 8


def leg_problem(N, seed, y_box=False, obj_scale=None):
    """A leg of N nodes that 11.5 m/s over the ground covers in (N - 1) H0 seconds, end poses drawn from `seed` -> oracle Problem,
    scenario row, the bowed start of nlp_steps_ref._start, the leg's length."""
    import nlp_steps_ref as S
    L = 11.5 * H0 * (N - 1)
    rng = np.random.default_rng([N, seed])
    p0 = (0.0, 0.0, rng.uniform(-0.3, 0.3)); p1 = (L * rng.uniform(0.93, 1.0), 0.12 * L * rng.uniform(-1, 1), rng.uniform(-0.3, 0.3))
    kw = dict(vsp=12.0, kv=5.0, kphi=1.0, obj_scale=(10.0 * N if N <= 5 else float(N) / 4) if obj_scale is None else obj_scale,
              phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0)
    if y_box:                                    # (the way over step_discs' first disc, whose top is at most 0.117 L from the axis, stays open)
        kw.update(y_box=(min(0.0, p1[1]) - 0.02 * L, max(0.0, p1[1]) + 0.14 * L))
    pb = nlp.Problem(N, H0, p0, p1, **kw)
    W0 = S._start(p0, p1, N, int(rng.integers(1 << 30)))
    return pb, S.scenario_row(pb), W0, L


def pad(discs):
    """(MAX_KEEP or fewer rows) -> the table of one problem, absent rows (R = 0) behind"""
    out = np.zeros((MAX_KEEP, 3))
    out[:len(discs)] = discs
    return out


STEP_N = (3, 5, 17, 64, 65, 121, 122, 129)
STEP_TAGS = ('bind', 'shear', 'two', 'many')
STEP_FIELD = 'shear'
STEP_T_START = 0.0
# (disc radius as a share of the leg, seed) of a case.  Chosen on the CPU with the statement alone (nlp_steps_ref.check): the largest
# radius of 9, 8, 7, 6 % (3 and 5 nodes: 9, 7, 5, 3 %) and then the first seed, counted from 0, at which the case is determined within
# nlp_steps_ref.TOL_CAP, keeps stepping after every budget and binds inside the budgets (a dual of 1 at least).  A disc that binds hard
# makes the Newton matrix indefinite before damping (the - z I term) and its ratio test cuts most early steps; on a short leg the
# one-ulp floor of the statement is then 1e-10 .. 4e-9, not 1e-12 -- such an input is not determined and is replaced, which here means
# a smaller disc.  At 3 and 5 nodes the first inner problem is solved within 8 steps at every candidate: the budget (8, 1) ends on the
# convergence test (tests/test_nlp_keepout_cpu.py says which checks it is held to), as in tests/nlp_free_ref.py.  Not listed: (0.09, 0).
STEP_CASES = {(3, 'bind'): (0.05, 3), (3, 'shear'): (0.05, 1), (3, 'two'): (0.05, 10), (3, 'many'): (0.09, 2),
              (5, 'bind'): (0.05, 0), (5, 'shear'): (0.07, 3), (5, 'two'): (0.09, 4),
              (17, 'bind'): (0.07, 7), (17, 'shear'): (0.07, 2), (17, 'two'): (0.07, 3),
              (64, 'bind'): (0.06, 3), (64, 'shear'): (0.07, 5), (64, 'two'): (0.07, 3),
              (65, 'bind'): (0.07, 7), (65, 'shear'): (0.07, 5), (65, 'two'): (0.07, 2),
              (121, 'bind'): (0.09, 3), (121, 'shear'): (0.09, 7), (121, 'two'): (0.09, 2), (121, 'many'): (0.09, 4),
              (122, 'bind'): (0.09, 6), (122, 'shear'): (0.09, 1),
              (129, 'shear'): (0.09, 4), (129, 'two'): (0.09, 5), (129, 'many'): (0.09, 1)}


def step_discs(tag, pb, L, Rf=0.09):
    """The discs of a step case: a binding disc 0.3 R off the leg's axis at its middle; the same disc; two overlapping discs; MAX_KEEP
    rows of which two are absent and the rest far away."""
    mid = 0.5 * (pb.p0[:2] + pb.p1[:2]); leg = pb.p1[:2] - pb.p0[:2]; ll = float(np.hypot(*leg))
    nrm = np.array([-leg[1], leg[0]]) / ll; ax = leg / ll
    R = max(Rf * L, Rf)                          # (the start's bow of 8 % of the leg reaches into it: the start rule moves those nodes out)
    c = mid + 0.3 * R * nrm
    if tag in ('bind', 'shear'):
        return pad([(c[0], c[1], R)])
    if tag == 'two':
        c2 = c - 1.5 * R * nrm + 0.1 * R * ax     # (below the first one: the near side is closed)
        return pad([(c[0], c[1], R), (c2[0], c2[1], R)])
    far = [(mid[0] + (3.0 + k) * L * np.cos(1.1 * k), mid[1] + (3.0 + k) * L * np.sin(1.1 * k), 0.5 * R) for k in range(MAX_KEEP)]
    far[2] = (far[2][0], far[2][1], 0.0); far[5] = (far[5][0], far[5][1], 0.0)
    return pad(far)


def ext(W, info):
    """The iterate with the discs' duals under it: W (N, 5), then zk as rows of 5 (zero padded) -- what the step-by-step comparison measures."""
    z = info['zk'].reshape(-1)
    z = np.concatenate([z, np.zeros((-len(z)) % 5)])
    return np.concatenate([W, z.reshape(-1, 5)])


def steps_case(cid, prob, W0, discs):
    import nlp_steps_ref as S
    N = prob.pb.N
    nz = (len(discs) * N + 4) // 5

    def run(W0s, inner_max, outer_max):
        W, info = solve(prob, W0s[0][:N], discs, inner_max=inner_max, outer_max=outer_max)
        return ext(W, info)[None], dict(inner=(info['inner'],), status=(info['status'],), path=tuple(info['path']), raw=info)
    return S.Case(cid, np.concatenate([W0, np.zeros((nz, 5))])[None], run,
                  lambda W: (prob.cost(W), float(np.abs(prob.constraints(W)).max())))


@functools.lru_cache(maxsize=None)
def steps_launch(N):
    """d2d_nlp_solve_keepout, the launches of N nodes: constant wind ('bind', 'two', 'many') and the field ('shear') go in two device
    calls.  -> dict tag -> (case, row, discs (MAX_KEEP, 3), prob)."""
    import nlp_wind_ref as R
    out = {}
    for tag in STEP_TAGS:
        Rf, seed = STEP_CASES.get((N, tag), (0.09, 0))
        pb, r, W0, L = leg_problem(N, 100 * STEP_TAGS.index(tag) + seed, y_box=(tag == 'two'))
        prob = R.FieldProblem(pb, R.fields()[STEP_FIELD], STEP_T_START) if tag == 'shear' else Plain(pb)
        discs = step_discs(tag, pb, L, Rf)
        out[tag] = (steps_case(f'keep-{N}-{tag}', prob, W0, discs), r, discs, prob)
    return out


FULL_N = (17, 41, 121)


FULL_KOBS = 0.02


@functools.lru_cache(maxsize=None)
def full_launch(N):
    """Full solves at N nodes: a leg that VSP = 12 m/s covers in (N - 1) H0 seconds, so every detour costs and the disc binds.  A user's
    disc of radius 8 % of the leg (1 % at 17 nodes) across it, its centre 0.3 r to the left of the axis, margin a quarter (a half) of that, lowered with
    lowered_radius; and the same with a second disc that closes the near (right) side, from a start bowed to the left.  The rows carry
    the first disc as a SOFT kind-1 obstacle too (weight FULL_KOBS): the soft-cost solve of the same rows is the comparison.
    -> list of (prob, row, W0, discs (MAX_KEEP, 3), (c, r, margin) of the first disc)."""
    import nlp_steps_ref as S
    out = []
    L = 12.0 * H0 * (N - 1)
    for two in (False, True):
        p0 = (0.0, 0.0, 0.1); p1 = (0.995 * L, 0.04 * L, -0.1)
        leg = np.array(p1[:2]) - np.array(p0[:2]); ll = float(np.hypot(*leg))
        nrm = np.array([-leg[1], leg[0]]) / ll
        mid = 0.5 * (np.array(p0[:2]) + np.array(p1[:2]))
        # (17 nodes are 1.6 s: the bank limit leaves no time for a detour of 8 % of the leg -- the statement stalls there -- so the disc
        # is 1 % of it and the lowered radius is mostly the chord term)
        ru, margin = (0.08 * L, 0.02 * L) if N >= 41 else (0.01 * L, 0.005 * L)
        c = mid + (0.3 * ru if N >= 41 else 0.025 * L) * nrm       # (17 nodes: on the bow that the end headings give the free plan)
        ob = [(c[0], c[1], ru)]
        pb = nlp.Problem(N, H0, p0, p1, vsp=12.0, kv=5.0, kphi=1.0, obj_scale=1.0, phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0,
                         obstacles=ob, kobs=FULL_KOBS, obs_kind=1)
        R = lowered_radius(ru, margin, pb.hi[1, 4], pb.h)
        discs = [(c[0], c[1], R)]
        t = np.linspace(0.0, 1.0, N)
        W0 = np.stack([p0[0] + t * leg[0], p0[1] + t * leg[1], np.full(N, np.arctan2(leg[1], leg[0])), np.zeros(N), np.full(N, 12.0)], 1)
        if two:
            c2 = c - 1.9 * R * nrm
            discs.append((c2[0], c2[1], R))
            W0[:, :2] += (0.12 * L * np.sin(np.pi * t))[:, None] * nrm
        out.append((Plain(pb), S.scenario_row(pb, ob, FULL_KOBS, 0), W0, pad(discs), (c, ru, margin)))
    return out


ARB_N = (5, 9, 17)


def arbiter_problem(N, two):
    """A case of tests/golden/nlp_keepout_slsqp.npz: the leg of full_launch at N nodes with one disc (R = 3 % of the leg) whose centre is
    0.3 R to the left of the leg's axis -- not on it: a leg aimed at a centre is a symmetric saddle for both solvers -- and, with `two`,
    a second one that closes the near (right) side, from the straight line bowed to the left by 6 % of the leg.  At 5 nodes the picture
    is mirrored (centre to the right, second disc on the left, bow to the right): with three interior nodes and the barrier's first
    parameter 0.1 against g ~ R^2 = 0.02 the central path leaves the start's side of so small a disc for the side of the free plan's
    bow (left, the end headings), where SLSQP, which knows no barrier, stays put -- two local minima, costs 9.52 and 10.31; mirrored,
    the start's side is the bow's and both solvers end there.
    -> oracle Problem, scenario row, W0, discs (n, 3)."""
    import nlp_steps_ref as S
    L = 12.0 * H0 * (N - 1)
    a = 0.1 * (N - 1) / 16.0                      # (end headings that the bank limit can join in (N - 1) H0 seconds at every N)
    p0 = (0.0, 0.0, 0.04 + a); p1 = (0.995 * L, 0.04 * L, 0.04 - a)
    leg = np.array(p1[:2]) - np.array(p0[:2]); ll = float(np.hypot(*leg))
    nrm = np.array([-leg[1], leg[0]]) / ll
    mid = 0.5 * (np.array(p0[:2]) + np.array(p1[:2]))
    R = 0.03 * L
    sd = 1.0 if N > 5 else -1.0                   # (5 nodes: mirrored -- see the docstring)
    nrm = sd * nrm
    c = mid + 0.3 * R * nrm
    pb = nlp.Problem(N, H0, p0, p1, vsp=12.0, kv=5.0, kphi=1.0, obj_scale=float(N), phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0)
    discs = [(c[0], c[1], R)]
    t = np.linspace(0.0, 1.0, N)
    W0 = np.stack([p0[0] + t * leg[0], p0[1] + t * leg[1], np.full(N, np.arctan2(leg[1], leg[0])), np.zeros(N), np.full(N, 12.0)], 1)
    if two:
        c2 = c - 1.9 * R * nrm
        discs.append((c2[0], c2[1], R))
        W0[:, :2] += (0.06 * L * np.sin(np.pi * t))[:, None] * nrm
    return pb, S.scenario_row(pb), W0, np.array(discs)
