"""CPU statement of the collocation solver INSIDE a convex polygon (include/d2d.h d2d_nlp_solve_fence; test infrastructure only).

It is tests/nlp_keepout_ref.py's statement -- oracle/nlp.py's augmented Lagrangian, primal-dual log barrier and damped Newton steps, with
the hard discs of d2d_nlp_solve_keepout -- with one more family of node inequalities: for every interior node i (1 .. N-2) and edge
k = (ax, ay, b, kap), a the outward unit normal, a row with ax = ay = 0 absent,

    g_ik = b - (ax x_i + ay y_i) > 0,        grad g = -a,  no second derivative,   s = the step of (x_i, y_i)

each with a dual z_ik > 0 that is treated exactly like the box duals and the discs':

  merit          - mub sum log g  (one log per node, of the product over the edges, beside the discs' log); +inf when any g <= 0
  stationarity   rows of (x_i, y_i):  ... + sum_k z a
  complementarity |z g - mub|, joined into err
  right-hand side the same rows with mub / g in the place of z:  - sum_k (mub / g) a
  Newton block   (x, y) corner of node i's diagonal block, half convention:  1/2 (z / g) a a^T  -- positive semidefinite
  dual step      dz = (mub + z a.s) / g - z;  ratio test and clip to [mub / (1e10 g), 1e10 mub / g] as the box duals
  primal ratio   linear and exact: a <= tau g / (a.s) where a.s > 0
  start          after the box push and the discs' rule (nlp_keepout_ref.start's loop), two passes over the edges in index order: a free
                 node with g_k < kap_k moves along -a_k to g_k = kap_k; then the box push again on x and y
  refusals       a non-finite entry, | |a| - 1 | > 1e-12 or kap <= 0 on a present edge, an end pose with g <= 0, a free node with any
                 g <= 0 (edge or disc) after the start rules -- and what nlp_keepout_ref refuses: status 3, NaN cost, W untouched

The feasible set of the edges is convex: the polyline between feasible nodes is feasible (segment_inside; no chord inflation).
The loop is oracle.nlp.solve_general with two families, nlp_keepout_ref.Discs before the family Edges that this file supplies, beside the
edges' start rule and refusals.  With no edge present solve() hands the problem to nlp_keepout_ref.solve, and is so oracle.nlp.solve
without discs.
"""
import functools

import numpy as np

import nlp_keepout_ref as K
from oracle import nlp

NV = nlp.NV
ST_NONFINITE = K.ST_NONFINITE
MAX_FENCE = 8
Plain = K.Plain
H0 = K.H0


def present(edges):
    return (edges[:, 0] != 0.0) | (edges[:, 1] != 0.0)


def g_values(W, edges):
    """(n, N) g of every (edge, node)"""
    return edges[:, 2, None] - (edges[:, 0, None] * W[None, :, 0] + edges[:, 1, None] * W[None, :, 1])


def segment_inside(edges, p, q):
    """The smallest g over the segment p -> q and the edges: g is linear along it, so the smaller of the two ends' -- the convexity
    guarantee in one line."""
    return float(min(g_values(np.array([p, q], float), edges).min(), np.inf))


def _disc_rule(pb, W, discs):
    """nlp_keepout_ref's rule for the discs, without its closing box push (the edges' rule comes first)."""
    return K.disc_rule(pb, W, *K.constant_centres(discs, pb.N))


def start(pb, W, discs, edges):
    """The start rules on a W that has had the box push: the discs' rule, the edges' rule, then the box push again on x and y."""
    W = _disc_rule(pb, W, discs) if len(discs) else W.copy()
    for i in range(1, pb.N - 1):
        x, y = W[i, 0], W[i, 1]
        for _pass in range(2):
            for ax, ay, b, kap in edges:
                if ax == 0.0 and ay == 0.0:
                    continue
                g = b - (ax * x + ay * y)
                if g < kap:
                    t = kap - g
                    x, y = x - t * ax, y - t * ay
        W[i, 0], W[i, 1] = x, y
    return K.push_xy(pb, W)


def refused(pb, discs, edges, Wp):
    """discs or edges unusable for this problem (Wp: the guess after the first box push)?"""
    if len(discs):
        if not np.isfinite(discs).all() or K.refused(pb, discs, K.start(pb, Wp, discs)):
            return True
    if not len(edges):
        return False
    if not np.isfinite(edges).all():
        return True
    act = edges[present(edges)]
    if not len(act):
        return False
    if (np.abs(np.sqrt(act[:, 0] * act[:, 0] + act[:, 1] * act[:, 1]) - 1.0) > 1e-12).any() or (act[:, 3] <= 0.0).any():
        return True
    if (g_values(np.array([pb.p0, pb.p1]), act) <= 0.0).any():
        return True
    W = start(pb, Wp, discs, edges)
    if (g_values(W[1:-1], act) <= 0.0).any():
        return True
    dact = discs[discs[:, 2] > 0.0] if len(discs) else discs
    return bool(len(dact) and (K.g_values(W[1:-1], dact)[0] <= 0.0).any())


def barrier_value(W, act, mub):
    """- mub sum log g over the interior nodes (one log per node, of the product over the edges); +inf when a g <= 0."""
    g = g_values(W[1:-1], act)
    if (g <= 0.0).any():
        return np.inf
    return -mub * float(np.sum(np.log(np.prod(g, axis=0))))


def barrier_terms(W, act, zf, mub):
    """What the loop adds for the edges at (W, zf): rhs (N, 2) [full convention, the negative merit gradient with mub / g], the stationarity
    term (N, 2) and the half-convention 2x2 blocks (N, 2, 2)."""
    N = len(W)
    g = g_values(W[1:-1], act)
    ax, ay = act[:, 0, None], act[:, 1, None]
    mg, zg = mub / g, 0.5 * (zf / g)
    rhs = np.zeros((N, 2)); st = np.zeros((N, 2)); blk = np.zeros((N, 2, 2))
    rhs[1:-1, 0] = -np.sum(mg * ax, axis=0); rhs[1:-1, 1] = -np.sum(mg * ay, axis=0)
    st[1:-1, 0] = np.sum(zf * ax, axis=0); st[1:-1, 1] = np.sum(zf * ay, axis=0)
    blk[1:-1, 0, 0] = np.sum(zg * ax * ax, axis=0); blk[1:-1, 1, 1] = np.sum(zg * ay * ay, axis=0)
    blk[1:-1, 0, 1] = blk[1:-1, 1, 0] = np.sum(zg * ax * ay, axis=0)
    return rhs, st, blk


class Edges:
    """The family of edges that oracle.nlp.solve_general asks for: the present rows of edges (n, 4)."""

    def __init__(self, edges):
        self.n = len(edges)
        self.ja = np.flatnonzero(present(edges))
        self.act = edges[self.ja]

    def __len__(self):
        return len(self.ja)

    def g(self, W):
        return g_values(W[1:-1], self.act)

    def barrier_value(self, W, mub):
        return barrier_value(W, self.act, mub)

    def barrier_terms(self, W, z, mub):
        return barrier_terms(W, self.act, z, mub)

    def _as(self, dw):
        """a.s at the interior nodes"""
        return self.act[:, 0, None] * dw[1:-1, 0] + self.act[:, 1, None] * dw[1:-1, 1]

    def ratio(self, W, dw, tau):
        as_ = self._as(dw)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(as_ > 0, tau * self.g(W) / as_, np.inf)

    def dual_step(self, W, dw, z, mub):
        return (mub + z * self._as(dw)) / self.g(W) - z

    def scatter(self, z, N):
        """the duals (n_present, N - 2) -> zf (n, N): 0 at the end nodes and for absent edges"""
        zfull = np.zeros((self.n, N))
        zfull[self.ja, 1:-1] = z
        return zfull


def solve(prob, W0, discs, edges, rho0=nlp.RHO0, inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX, feas_tol=nlp.FEAS_TOL, opt_tol=nlp.OPT_TOL):
    """nlp_keepout_ref.solve inside the edges (n, 4) = (ax, ay, b, kap) (ax = ay = 0: absent).  Returns W, info of nlp_keepout_ref.solve
    plus zf (n, N): the edges' duals (0 at the end nodes and for absent edges).  A refused problem: W0 itself, status 3, NaN cost and feas."""
    pb = prob.pb
    discs = np.asarray(discs, float).reshape(-1, 3)
    edges = np.asarray(edges, float).reshape(-1, 4)
    schedule = dict(rho0=rho0, inner_max=inner_max, outer_max=outer_max, feas_tol=feas_tol, opt_tol=opt_tol)
    if not len(edges) or (np.isfinite(edges).all() and not present(edges).any()):
        W, info = K.solve(prob, W0, discs, **schedule)
        info['zf'] = np.zeros((len(edges), pb.N))
        return W, info
    W = nlp.interior_start(pb, W0)
    if refused(pb, discs, edges, W):
        return np.asarray(W0, float).copy(), dict(cost=np.nan, feas=np.nan, outer=0, inner=0, status=ST_NONFINITE, path=[],
                                                  zk=np.zeros((len(discs), pb.N)), zf=np.zeros((len(edges), pb.N)))
    W = start(pb, W, discs, edges)
    fd, fe = K.Discs(*K.constant_centres(discs, pb.N)), Edges(edges)
    W, info, end = nlp.solve_general(prob, W, families=(fd, fe), started=True, **schedule)
    info.update(zk=fd.scatter(end['z'][0], pb.N), zf=fe.scatter(end['z'][1], pb.N), mub=end['mub'])
    return W, info


# ---- geometry of the cases ---------------------------------------------------------------------------------------------------------
def leg_frame(pb):
    """p0, the unit vector along the leg p0 -> p1, its left normal and the leg's length"""
    p0 = np.asarray(pb.p0[:2], float); leg = np.asarray(pb.p1[:2], float) - p0; ll = float(np.hypot(*leg))
    ax = leg / ll
    return p0, ax, np.array([-ax[1], ax[0]]), ll


def corridor(pb, left, right, back, ahead):
    """Vertices (counter-clockwise) of the rectangle round the leg: `left` / `right` of its axis, `back` behind p0, `ahead` beyond p1."""
    p0, ax, nrm, ll = leg_frame(pb)
    return np.array([p0 - back * ax - right * nrm, p0 + (ll + ahead) * ax - right * nrm, p0 + (ll + ahead) * ax + left * nrm, p0 - back * ax + left * nrm])


def fence_rows(vertices, margin=0.0):
    import d2d.opty_utils as ou
    return ou.GeoFence(vertices, margin).lowered()


def pad(edges):
    """(MAX_FENCE or fewer rows) -> the table of one problem, absent rows (zeros) behind"""
    out = np.zeros((MAX_FENCE, 4))
    out[:len(edges)] = edges
    return out


def lateral(pb, W):
    """the nodes' offsets to the left of the leg's axis"""
    p0, _, nrm, _ = leg_frame(pb)
    return (W[:, :2] - p0) @ nrm


def ext(W, info):
    """The iterate with the discs' and the edges' duals under it, as rows of 5 (zero padded): what the step-by-step comparison measures."""
    z = np.concatenate([info['zk'].reshape(-1), info['zf'].reshape(-1)])
    z = np.concatenate([z, np.zeros((-len(z)) % 5)])
    return np.concatenate([W, z.reshape(-1, 5)])


# ---- step by step: tests/test_nlp_fence_cpu.py, tests/test_gpu_nlp_fence.py ----------------------------------------------------------
STEP_N = (3, 5, 17, 64, 65, 121)
STEP_TAGS = ('bind', 'many', 'disc', 'shear')
STEP_FIELD = 'shear'
STEP_T_START = 0.0
STEP_EDGE = 0.03        # the binding edge lies this share of the leg to the left of its axis: inside the start's bow of 8 %, which the start rule moves
# seed of a case, chosen on the CPU with the statement alone (nlp_steps_ref.check): the first seed, counted from 0, at which the case is
# determined within nlp_steps_ref.TOL_CAP, keeps stepping after every budget and has the edge act (tests/test_nlp_fence_cpu.py says how
# that is measured).  Not listed: 0.
STEP_SEEDS = {(3, 'many'): 3, (3, 'disc'): 1, (3, 'shear'): 1, (5, 'many'): 3, (5, 'disc'): 1, (5, 'shear'): 2,
              (64, 'bind'): 2, (64, 'disc'): 3, (65, 'many'): 1, (65, 'disc'): 2}
STEP_DISC = 0.05        # the disc of the 'disc' case: this share of the leg in radius, 0.3 R to the left of the axis at mid-leg


def step_tables(tag, pb, L):
    """discs (MAX_KEEP, 3) and edges (MAX_FENCE, 4) of a step case.  'bind', 'shear': the rectangle round the leg whose left edge is
    STEP_EDGE L from the axis (the other three stand far off).  'many': MAX_FENCE rows -- that rectangle's four, two absent rows (2 and 5)
    and two more edges far away.  'disc': the rectangle with its left edge behind a hard disc, 0.03 L beyond the disc's far side."""
    discs = np.zeros((K.MAX_KEEP, 3))
    left = STEP_EDGE * L
    if tag == 'disc':
        discs = K.step_discs('bind', pb, L, STEP_DISC)
        left = (1.3 * STEP_DISC + 0.03) * L
    rect = fence_rows(corridor(pb, left, 2.0 * L, 0.5 * L, 0.5 * L))
    if tag != 'many':
        return discs, pad(rect)
    p0, ax, nrm, ll = leg_frame(pb)
    far = []
    for th in (0.7, -2.1):                       # two more half-planes, 3 L from mid-leg
        a = np.cos(th) * ax + np.sin(th) * nrm
        far.append((a[0], a[1], float(a @ (p0 + 0.5 * ll * ax)) + 3.0 * L, 0.05 * L))
    z = (0.0, 0.0, 0.0, 0.0)
    return discs, np.array([rect[0], rect[1], z, rect[2], far[0], z, rect[3], far[1]])


def steps_case(cid, prob, W0, discs, edges):
    import nlp_steps_ref as S
    N = prob.pb.N
    nz = ((len(discs) + len(edges)) * N + 4) // 5

    def run(W0s, inner_max, outer_max):
        W, info = solve(prob, W0s[0][:N], discs, edges, inner_max=inner_max, outer_max=outer_max)
        return ext(W, info)[None], dict(inner=(info['inner'],), status=(info['status'],), path=tuple(info['path']), raw=info)
    return S.Case(cid, np.concatenate([W0, np.zeros((nz, 5))])[None], run,
                  lambda W: (prob.cost(W), float(np.abs(prob.constraints(W)).max())))


@functools.lru_cache(maxsize=None)
def steps_launch(N):
    """d2d_nlp_solve_fence, the launches of N nodes: constant wind ('bind', 'many', 'disc') and the field ('shear') go in two device
    calls.  -> dict tag -> (case, row, discs (MAX_KEEP, 3), edges (MAX_FENCE, 4), prob)."""
    import nlp_wind_ref as R
    out = {}
    for tag in STEP_TAGS:
        seed = STEP_SEEDS.get((N, tag), 0)
        pb, r, W0, L = K.leg_problem(N, 1000 + 100 * STEP_TAGS.index(tag) + seed)
        prob = R.FieldProblem(pb, R.fields()[STEP_FIELD], STEP_T_START) if tag == 'shear' else Plain(pb)
        discs, edges = step_tables(tag, pb, L)
        out[tag] = (steps_case(f'fence-{N}-{tag}', prob, W0, discs, edges), r, discs, edges, prob)
    return out


# ---- the independent arbiter: tests/golden/nlp_fence_slsqp.npz (tests/golden/make_nlp_fence_golden.py) -------------------------------
ARB_CASES = ('cut-5', 'cut-9', 'cut-17', 'roof-9', 'mixed-17')
# The share of the free plan's bow that the corridor's left edge leaves.  At 5 nodes a half is infeasible for the statement (STALLED) and
# for SLSQP alike (three interior nodes 2.4 m apart cannot turn that sharply); tried on the CPU: 0.6 infeasible for both, 0.7 SLSQP succeeds
# and the statement ends at its iteration cap 6.5e-8 off, 0.8 CONVERGED after 555 steps (2.0e-9 off), 0.9 CONVERGED after 21 (7.6e-9 off,
# the edge's dual 2.1): 0.9.
ARB_CUT = {5: 0.9, 9: 0.5, 17: 0.5}


def leg(N):
    """nlp_keepout_ref.arbiter_problem(N, False)'s leg, row and straight start up to 41 nodes.  Beyond, the same construction with the end
    headings held at 41 nodes' 0.04 +- 0.25 rad: the arbiter's rule, +- 0.1 (N - 1) / 16, gives +- 0.75 rad at 121 nodes, and from such a leg
    the statement's step count inside a corridor changes when its start moves by an ulp (78 / 79 steps, and up to 2310 at other cuts)."""
    if N <= 41:
        return K.arbiter_problem(N, False)[:3]
    import nlp_steps_ref as S
    L = 12.0 * H0 * (N - 1)
    p0 = (0.0, 0.0, 0.04 + 0.25); p1 = (0.995 * L, 0.04 * L, 0.04 - 0.25)
    pb = nlp.Problem(N, H0, p0, p1, vsp=12.0, kv=5.0, kphi=1.0, obj_scale=float(N), phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0)
    t = np.linspace(0.0, 1.0, N)
    d = np.array(p1[:2]) - np.array(p0[:2])
    W0 = np.stack([p0[0] + t * d[0], p0[1] + t * d[1], np.full(N, np.arctan2(d[1], d[0])), np.zeros(N), np.full(N, 12.0)], 1)
    return pb, S.scenario_row(pb), W0


@functools.lru_cache(maxsize=None)
def free_plan(N):
    """The leg of leg(N), its free plan (the statement without discs or edges) and the largest offset of that plan to the left of the
    leg's axis: the bow that the end headings give it."""
    pb, row, W0 = leg(N)
    W, info = K.solve(Plain(pb), W0, np.zeros((0, 3)))
    assert info['status'] == 1
    return pb, row, W0, W, float(lateral(pb, W).max())


def arbiter_problem(name):
    """A case of the golden file -> oracle Problem, scenario row, W0, discs (n, 3), edges (n, 4).
    'cut-N': the rectangle round the leg whose left edge lies at ARB_CUT[N] of the free plan's bow; the other three edges stand far off.
    'roof-9': the left edge replaced by two that meet above mid-leg at 0.7 of the bow and fall to 0.4 of it at the polygon's ends, 10 % of the
    leg behind p0 and beyond p1: both cut the bow, on either side of the apex (duals 5.9 and 3.6e-2; apex 0.6 / ends 0.2 is infeasible
    for the statement and for SLSQP alike, and at 0.8 / 0.5, 0.75 / 0.3, 0.85 / 0.6 and 0.9 / 0.5 only the edge beyond the apex binds).
    'mixed-17': 'cut-17' with one hard disc on another part of the leg: its centre at 0.3 of the leg's length, 0.5 R inside the left edge,
    R = 3 % of the leg (more than the bow), so that the plan passes below it and comes back up against the edge beyond mid-leg: both carry
    duals (edge 38, disc 76).  Tried on the CPU, centre relative to the edge: 0.3 R beyond it, on it (also at 0.2 and 0.25 of the leg, R 2 %)
    and 0.2 R inside -- the detour below the disc then keeps the plan off the edge (its dual < 2e-8), only the disc binds."""
    kind, N = name.split('-'); N = int(N)
    pb, row, W0, _, bow = free_plan(N)
    p0, ax, nrm, ll = leg_frame(pb)
    discs = np.zeros((0, 3))
    if kind == 'roof':
        v = [p0 - 0.1 * ll * ax - ll * nrm, p0 + 1.1 * ll * ax - ll * nrm, p0 + 1.1 * ll * ax + 0.4 * bow * nrm, p0 + 0.5 * ll * ax + 0.7 * bow * nrm,
             p0 - 0.1 * ll * ax + 0.4 * bow * nrm]
        return pb, row, W0, discs, fence_rows(np.array(v))
    left = ARB_CUT[N] * bow
    edges = fence_rows(corridor(pb, left, ll, 0.5 * ll, 0.5 * ll))
    if kind == 'mixed':
        R = 0.03 * ll
        c = p0 + 0.3 * ll * ax + (left - 0.5 * R) * nrm
        discs = np.array([[c[0], c[1], R]])
    return pb, row, W0, discs, edges


# ---- full solves: tests/test_nlp_fence_cpu.py, tests/test_gpu_nlp_fence.py ------------------------------------------------------------
FULL_N = (17, 41, 121)
FULL_MARGIN = 0.01          # the GeoFence's margin, as a share of the leg
# per node count: the share of the free plan's bow that the lowered left edge leaves, and the hard disc's radius as a share of the leg.
# Chosen on the CPU so that the statement converges with a step count that does not change when its start moves by an ulp
# (tests/test_nlp_fence_cpu.py) and, in 'both', edge AND disc end with duals that count (17: 38 / 76, 41: 0.54 / 1.5, 121: 0.23 / 0.11).
# Tried and dropped: 41 nodes with R 3 % (the detour below the disc keeps the plan off the edge, its dual 4e-9; so does 2 %); 121 nodes with
# R 2 % (the edge's dual 0.026 at a share of 0.5, 0 at 0.7); 121 nodes on the arbiter's own leg, see leg().
FULL_PAR = {17: (0.5, 0.03), 41: (0.5, 0.01), 121: (0.5, 0.005)}


@functools.lru_cache(maxsize=None)
def full_launch(N):
    """Full solves at N nodes on leg(N), inside a d2d.opty_utils.GeoFence with margin
    FULL_MARGIN L -- the rectangle round the leg, three sides far off, the left one so that the LOWERED edge (margin taken off) leaves the
    share FULL_PAR[N][0] of the free plan's bow:
      'fence': no hard disc;
      'both':  one hard disc as in the arbiter's 'mixed' case: R = FULL_PAR[N][1] of the leg, its centre at 0.3 of the leg's length and 0.5 R inside the
               lowered edge; the plan passes below it and comes back up against the edge.
    -> list of (prob, row, W0, discs (MAX_KEEP, 3), edges (MAX_FENCE, 4), GeoFence)."""
    import d2d.opty_utils as ou
    pb, row, W0, _, bow = free_plan(N)
    p0, ax, nrm, ll = leg_frame(pb)
    m = FULL_MARGIN * ll
    cut, Rf = FULL_PAR[N]
    gf = ou.GeoFence(corridor(pb, cut * bow + m, ll, 0.5 * ll, 0.5 * ll), m)
    R = Rf * ll
    c = p0 + 0.3 * ll * ax + (cut * bow - 0.5 * R) * nrm
    return [(Plain(pb), row, W0, np.zeros((K.MAX_KEEP, 3)), pad(gf.lowered()), gf),
            (Plain(pb), row, W0, K.pad([(c[0], c[1], R)]), pad(gf.lowered()), gf)]


# ---- groups: d2d_nlp_solve_groups_fence (tests/test_gpu_groups_fence.py) ---------------------------------------------------------------
GROUP_N = (17, 41)
GROUP_SWEEPS = 24
GROUP_T_START = 1.0


def problem_of(pb, field=None, t_start=0.0):
    import nlp_wind_ref as Rw
    return Plain(pb) if field is None else Rw.FieldProblem(pb, field, t_start)


def solve_groups(rows, edges, W0s, field=None, t_start=0.0, max_sweeps=12, tol=1e-7, N=None, h=None, **kw):
    """One scenario of len(rows) aircraft with the partner sets of the rows' SC_PMASK, every aircraft inside the scenario's edges (n, 4); no
    hard discs.  Returns Ws, infos, sweeps, moved of nlp_groups_pairs_ref.solve_groups; a scenario with an aircraft that is refused
    before its first solve is refused whole: the guesses, status 3 and NaN for every aircraft, 0 sweeps.  A later turn that cannot
    start leaves that aircraft's nodes and reports it alone."""
    import nlp_groups_pairs_ref as P
    N = len(W0s[0]) if N is None else N
    h = H0 if h is None else h
    edges = np.asarray(edges, float).reshape(-1, 4)
    none = np.zeros((0, 3))
    pbs = [nlp.problem_from_row(r, N, h) for r in rows]

    def inner(a, pb, W0):
        return solve(problem_of(pb, field, t_start), W0, none, edges, **kw)
    if len(edges):
        for pb, W0 in zip(pbs, W0s):                 # the scenario's refusal: every aircraft's start, before the first solve
            fixed, hasL, hasU = nlp._barrier_sets(pb)
            W = np.asarray(W0, float).copy()
            W[:, :2] = K._box_push(W[:, :2], pb.lo[:, :2], pb.hi[:, :2], hasL[:, :2], hasU[:, :2])
            if refused(pb, none, edges, W):
                bad = dict(cost=np.nan, feas=np.nan, inner=0, status=ST_NONFINITE, zf=np.zeros((len(edges), N)))
                return [np.asarray(w, float).copy() for w in W0s], [dict(bad) for _ in rows], 0, 0.0
    return P.solve_groups(pbs, W0s, inner, P.masks_of(rows), max_sweeps=max_sweeps, tol=tol)


def pair_scenario(N, gap=9.0, room=0.2, top=5.0):
    """nlp_keepout_moving_ref.pair_scenario's pair -- two aircraft side by side `gap` m apart (inside rcol = 10 m: CostCollision acts along
    the leg), aircraft 1 to the right of aircraft 0, masks of the pair (0, 1) -- without its disc, inside a rectangle whose right edge
    lies `room` m on the outer side of aircraft 1's leg: the collision term pushes aircraft 1 against it.  The left edge lies `top` m
    beyond aircraft 0's leg, the other two half a leg behind and beyond the end poses.  -> rows (2, SCEN_STRIDE), guesses, edges (4, 4)."""
    import nlp_keepout_moving_ref as KM
    rows, W0s, _ = KM.pair_scenario(N, gap)
    L = 12.0 * H0 * (N - 1)
    edges = fence_rows(np.array([(-0.5 * L, -gap - room), (1.5 * L, -gap - room), (1.5 * L, top), (-0.5 * L, top)]))
    return rows, W0s, edges
