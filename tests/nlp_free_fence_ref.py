"""CPU statement of the collocation solver with a FREE time step outside static hard discs and inside a convex polygon (include/d2d.h
d2d_nlp_solve_free_fence; test infrastructure only).

Nothing here is a solver of its own: the loop is oracle.nlp.solve_general, called with the two families of tests/nlp_fence_ref.py
(nlp_keepout_ref.Discs, then nlp_fence_ref.Edges) BESIDE the border of tests/nlp_free_ref.py (Border: u = 1 / h in its box, two duals,
the bordered solve) on a FreeProblem.  Discs and edges read (x, y) of the interior nodes alone, so the border column b, the scalar d and
the residual of the row of u gain no term; what the families add to the block-tridiagonal matrix A is in both solves of the Schur
complement, x0 = A^-1 r / 2 and y = A^-1 b.  The step length is the smallest of four ratio tests in solve_general's order: the box, the
discs' exact quadratic root, the edges' tau g / (a.s), u's.

  start      the box push (oracle.nlp.interior_start), the discs' rule, the edges' rule, the box push again on x and y
             (nlp_fence_ref.start); the step pushed strictly inside its box (nlp_free_ref.Border)
  refusals   what nlp_fence_ref.refused refuses: status 3, NaN cost, feas and h, W untouched.  (A bad row of the step's box is the
             kernel's to refuse, as in tests/nlp_free_ref.py: FreeProblem takes a usable box.)
  no tables  with no row of either table, solve() is nlp_free_ref.solve: its W and info bit for bit.
"""
import functools

import numpy as np

import nlp_fence_ref as E
import nlp_free_ref as F
import nlp_keepout_ref as K
from oracle import nlp

H0 = F.H0
ST_NONFINITE = K.ST_NONFINITE
MAX_KEEP, MAX_FENCE = K.MAX_KEEP, E.MAX_FENCE


def solve(fp, W0, h_start, discs, edges, rho0=nlp.RHO0, inner_max=nlp.INNER_MAX, outer_max=nlp.OUTER_MAX, feas_tol=nlp.FEAS_TOL,
          opt_tol=nlp.OPT_TOL):
    """nlp_free_ref.solve outside the discs (n, 3) = (cx, cy, R) (R <= 0: absent) and inside the edges (n, 4) = (ax, ay, b, kap)
    (ax = ay = 0: absent).  Returns W, info with the keys of both parents: those of oracle.nlp.solve, h, u, zu (the two duals of u),
    mult_last, zk (n_keep, N) and zf (n_edge, N) (0 at the end nodes and for absent rows), mub.  A refused problem: W0 itself, status 3,
    NaN cost, feas, h and u."""
    pb = fp.pb
    discs = np.asarray(discs, float).reshape(-1, 3)
    edges = np.asarray(edges, float).reshape(-1, 4)
    schedule = dict(rho0=rho0, inner_max=inner_max, outer_max=outer_max, feas_tol=feas_tol, opt_tol=opt_tol)
    if not len(discs) and not len(edges):
        W, info = F.solve(fp, W0, h_start, **schedule)
        info.update(zk=np.zeros((0, pb.N)), zf=np.zeros((0, pb.N)))
        return W, info
    W = nlp.interior_start(pb, W0)
    if E.refused(pb, discs, edges, W):
        return np.asarray(W0, float).copy(), dict(cost=np.nan, feas=np.nan, h=np.nan, u=np.nan, outer=0, inner=0, status=ST_NONFINITE, path=[],
                                                  zk=np.zeros((len(discs), pb.N)), zf=np.zeros((len(edges), pb.N)))
    W = E.start(pb, W, discs, edges)
    bd = F.Border(fp, h_start)
    fd, fe = K.Discs(*K.constant_centres(discs, pb.N)), E.Edges(edges)
    W, info, end = nlp.solve_general(fp, W, families=(fd, fe), border=bd, started=True, **schedule)
    info.update(h=1.0 / bd.u, u=bd.u, zu=(bd.zl, bd.zu), mult_last=2 * info['rho'] * (end['mu'] + fp.constraints(W, bd.u)),
                zk=fd.scatter(end['z'][0], pb.N), zf=fe.scatter(end['z'][1], pb.N), mub=end['mub'])
    return W, info


def fixed_solve(fp, W0, h, discs, edges, **schedule):
    """The same problem with the step FIXED at h: nlp_fence_ref.solve (d2d_nlp_solve_fence) on the Problem at that step."""
    return E.solve(E.Plain(fp.at(1.0 / h)), W0, discs, edges, **schedule)


def kkt_residual(fp, W, info, discs, edges):
    """nlp_free_ref.kkt_residual (the node rows and the row of u) with the families' terms in the stationarity rows of (x, y) of the
    interior nodes: - sum z 2 d for the discs, + sum z a for the edges, as the loop adds them (barrier_terms).  They are handed over on
    the upper duals' side, where the residual adds them.  -> largest stationarity residual, feasibility."""
    N = fp.pb.N
    discs = np.asarray(discs, float).reshape(-1, 3); edges = np.asarray(edges, float).reshape(-1, 4)
    st = np.zeros((N, nlp.NV))
    fd, fe = K.Discs(*K.constant_centres(discs, N)), E.Edges(edges)
    if len(fd):
        st[:, :2] += fd.barrier_terms(W, info['zk'][fd.ia][:, 1:-1], info['mub'])[1]
    if len(fe):
        st[:, :2] += fe.barrier_terms(W, info['zf'][fe.ja][:, 1:-1], info['mub'])[1]
    return F.kkt_residual(fp, W, info['h'], info['mult_last'], info['zL'], info['zU'] + st, info['zu'])


def free_rows(fps, h_start=0.0):
    return F.free_rows(fps, h_start)


def ext(W, info):
    """The iterate with its interval and the families' duals: W (N, 5), the row (h, u, 0, 0, 0), then zk and zf as rows of 5 (zero padded)
    -- what the step-by-step comparison measures."""
    z = np.concatenate([info['zk'].reshape(-1), info['zf'].reshape(-1)])
    z = np.concatenate([z, np.zeros((-len(z)) % 5)])
    return np.concatenate([W, [[info['h'], info['u'], 0.0, 0.0, 0.0]], z.reshape(-1, 5)])


def steps_case(cid, fp, W0, discs, edges, h_start=H0):
    """A nlp_steps_ref Case of one solve: the iterate is ext(W, info); the rows under the start are place holders."""
    import nlp_steps_ref as S
    N = fp.pb.N
    nz = 1 + ((len(discs) + len(edges)) * N + 4) // 5

    def run(W0s, inner_max, outer_max):
        W, info = solve(fp, W0s[0][:N], h_start, discs, edges, inner_max=inner_max, outer_max=outer_max)
        return ext(W, info)[None], dict(inner=(info['inner'],), status=(info['status'],), path=tuple(info['path']), raw=info)
    return S.Case(cid, np.concatenate([W0, np.zeros((nz, 5))])[None], run,
                  lambda W, h: (fp.cost(W, 1.0 / h), float(np.abs(fp.constraints(W, 1.0 / h)).max())))


# ---- step by step: tests/test_nlp_free_fence_cpu.py, tests/test_gpu_nlp_free_fence.py ------------------------------------------------
STEP_N = (3, 5, 17, 64, 65, 121, 122, 129)
STEP_TAGS = ('disc', 'edge', 'both', 'many')
STEP_KDUR = dict(disc=0.5, edge=0.0, both=2.0, many=0.5)
STEP_RADII = (0.09, 0.08, 0.07, 0.06, 0.05)
STEP_SEEDS = 16
# (disc radius as a share of the leg, seed) of a case, chosen on the CPU with the statement alone by the rule written above
# nlp_keepout_ref.STEP_CASES: the largest radius of 9, 8, 7, 6, 5 % and then the first seed, counted from 0 to 15, at which the case is
# determined within nlp_steps_ref.TOL_CAP, keeps stepping after every budget (nlp_steps_ref.check) and reaches a dual of at least 1 on a
# disc or an edge inside the budgets.  'edge' and 'many' carry no disc that binds: only the seed is searched (their radius entry is the
# far discs' of 'many', 9 %).  'many' holds nothing that CAN bind -- every present row is far away -- and is not asked for the dual.
# A cell that is not listed has NO such candidate and is left out of its launch; the conditions that the
# table must meet (three of four kinds at every node count, every kind at five node counts or more) are asserted in
# tests/test_nlp_free_fence_cpu.py.  tools/dev/nlp_free_fence_select.py prints this table.
STEP_CASES = {(3, 'disc'): (0.09, 5), (3, 'both'): (0.08, 10), (3, 'many'): (0.09, 5),
              (5, 'disc'): (0.06, 8), (5, 'edge'): (0.09, 2), (5, 'both'): (0.06, 4), (5, 'many'): (0.09, 0),
              (17, 'disc'): (0.07, 5), (17, 'edge'): (0.09, 2), (17, 'both'): (0.07, 13), (17, 'many'): (0.09, 0),
              (64, 'disc'): (0.07, 1), (64, 'edge'): (0.09, 0), (64, 'both'): (0.06, 6), (64, 'many'): (0.09, 2),
              (65, 'disc'): (0.06, 7), (65, 'edge'): (0.09, 2), (65, 'both'): (0.07, 2), (65, 'many'): (0.09, 0),
              (121, 'disc'): (0.09, 0), (121, 'edge'): (0.09, 0), (121, 'both'): (0.09, 7), (121, 'many'): (0.09, 9),
              (122, 'disc'): (0.09, 4), (122, 'edge'): (0.09, 0), (122, 'both'): (0.09, 2), (122, 'many'): (0.09, 2),
              (129, 'disc'): (0.09, 11), (129, 'edge'): (0.09, 3), (129, 'both'): (0.09, 0), (129, 'many'): (0.09, 1)}


def step_problem(N, tag, seed):
    """The leg of a step case: nlp_keepout_ref.leg_problem's (11.5 m/s over the ground, end poses and the bowed start drawn from the
    seed; 'both' with its y box), its step free in H0 * (0.5, 2.0) with the kind's weight of the duration.  -> FreeProblem, row, W0, L."""
    pb, r, W0, L = K.leg_problem(N, 2000 + 100 * STEP_TAGS.index(tag) + seed, y_box=(tag == 'both'))
    return F.FreeProblem(pb, 0.5 * H0, 2.0 * H0, STEP_KDUR[tag]), r, W0, L


STEP_CUT = 0.5          # 'edge': the share of the free plan's bow that the corridor's long edges leave


def step_corridor(fp, W0, L, narrow=False):
    """A rectangle round the leg whose long edge binds.  A convex set that holds both end poses holds the leg's axis, so an edge binds only
    where the end headings bow the plan: the plan of the same problem WITHOUT tables (nlp_free_ref.solve, the step free) is solved first,
    and the edge on the side of its larger bow leaves STEP_CUT of it.  narrow=False (the full solves): the other three edges stand far
    off.  narrow=True (the step kind 'edge'): a corridor in earnest, the opposite edge as close to the axis -- d2d.opty_utils.GeoFence
    then gives the start rule's kap as 1 % of that width, centimetres, so the nodes of the bowed start are moved to within centimetres
    of the edge and its terms weigh in the very first Newton steps, not only near the end of a solve.  None where the plan without
    tables does not converge or has no bow."""
    W, info = F.solve(fp, W0, H0)
    if info['status'] != 1:
        return None
    lat = E.lateral(fp.pb, W)
    up, dn = float(lat.max()), float(-lat.min())
    if not max(up, dn) > 0.0:
        return None
    far = STEP_CUT * max(up, dn) if narrow else 2.0 * L
    left, right = (STEP_CUT * up, far) if up >= dn else (far, STEP_CUT * dn)
    return E.fence_rows(E.corridor(fp.pb, left, right, 0.5 * L, 0.5 * L))


def step_tables(tag, fp, W0, L, Rf):
    """discs (MAX_KEEP, 3) and edges (MAX_FENCE, 4) of a step case.
    'disc': nlp_keepout_ref's binding disc (radius Rf L, 0.3 R to the left of the axis at mid-leg), every edge absent.
    'edge': step_corridor's narrow corridor (both long edges at STEP_CUT of the free plan's bow from the axis), every disc absent.
    'both': the binding disc behind the left edge of a rectangle, 0.03 L beyond the disc's far side (and the leg's y box).
    'many': MAX_KEEP discs of which two are absent and the rest far away; MAX_FENCE edges: a rectangle 2 L to either side of the leg, two
            absent rows (2 and 5) and two more half-planes 3 L from mid-leg -- every present row far away: the rolled loops run their full
            length and nothing can bind, so the selection does not ask this kind for a dual of 1 (nlp_keepout_ref's 'many' is the same)."""
    pb = fp.pb
    if tag == 'disc':
        return K.step_discs('bind', pb, L, Rf), np.zeros((MAX_FENCE, 4))
    if tag == 'both':
        left = (1.3 * Rf + 0.03) * L
        return K.step_discs('bind', pb, L, Rf), E.pad(E.fence_rows(E.corridor(pb, left, 2.0 * L, 0.5 * L, 0.5 * L)))
    if tag == 'edge':
        rect = step_corridor(fp, W0, L, narrow=True)
        return (None, None) if rect is None else (np.zeros((MAX_KEEP, 3)), E.pad(rect))
    rect = E.fence_rows(E.corridor(pb, 2.0 * L, 2.0 * L, 0.5 * L, 0.5 * L))
    p0, ax, nrm, ll = E.leg_frame(pb)
    far = []
    for th in (0.7, -2.1):
        a = np.cos(th) * ax + np.sin(th) * nrm
        far.append((a[0], a[1], float(a @ (p0 + 0.5 * ll * ax)) + 3.0 * L, 0.05 * L))
    z = (0.0, 0.0, 0.0, 0.0)
    return K.step_discs('many', pb, L, Rf), np.array([rect[0], rect[1], z, rect[2], far[0], z, rect[3], far[1]])


def step_candidate(N, tag, Rf, seed):
    """-> case, row, discs, edges, FreeProblem of one candidate of the selection (None: the corridor could not be built)"""
    fp, r, W0, L = step_problem(N, tag, seed)
    discs, edges = step_tables(tag, fp, W0, L, Rf)
    if discs is None:
        return None
    return steps_case(f'freefence-{N}-{tag}', fp, W0, discs, edges), r, discs, edges, fp


def step_complaints(case, N, budget):
    """nlp_steps_ref.check of a step case after a budget.  At 3 and 5 nodes the first inner problem is solved within 8 steps, so there the
    budget (8, 1) ends on the convergence test and is held to the tolerance and the path alone -- the rule above
    nlp_keepout_ref.STEP_CASES, as tests/test_nlp_keepout_cpu.py and tests/test_nlp_fence_cpu.py apply it."""
    import nlp_steps_ref as S
    bad = S.check(case, budget)
    if N <= 5 and budget == (8, 1):
        bad = [b for b in bad if b.startswith('tol') or b.startswith('the perturbed')]
    return bad


@functools.lru_cache(maxsize=None)
def steps_launch(N):
    """d2d_nlp_solve_free_fence, one launch of N nodes: the kinds of STEP_TAGS that STEP_CASES lists for N.
    -> dict tag -> (case, row, discs (MAX_KEEP, 3), edges (MAX_FENCE, 4), FreeProblem)."""
    return {tag: step_candidate(N, tag, *STEP_CASES[(N, tag)]) for tag in STEP_TAGS if (N, tag) in STEP_CASES}


# ---- the cases where only the free step answers ------------------------------------------------------------------------------------
VERIFIED = ((17, 0), (41, 0))          # (nodes, seed): the fixed step STALLS, the free step CONVERGES


def detour_problem(N, seed, k_dur=0.0, Rf=0.09, half=0.3):
    """A leg that 14.5 m/s covers in (N - 1) H0 seconds -- the aircraft's v_max is 15: no time to spare -- with nlp_keepout_ref's binding
    disc (Rf of the leg) across it, inside a corridor `half` of the leg to either side and a tenth of it behind and beyond the end
    poses, margin 0.  The detour round the disc does not fit the leg's (N - 1) H0 seconds at every seed.
    -> FreeProblem (step free in H0 * (0.5, 2.0)), row, W0, discs (MAX_KEEP, 3), edges (MAX_FENCE, 4)."""
    fp, r, W0 = F.leg_problem(N, seed, k_dur=k_dur, speed=14.5)
    L = 14.5 * H0 * (N - 1)
    discs = K.step_discs('bind', fp.pb, L, Rf=Rf)
    edges = E.pad(E.fence_rows(E.corridor(fp.pb, half * L, half * L, 0.1 * L, 0.1 * L)))
    return fp, r, W0, discs, edges


# ---- full solves ----------------------------------------------------------------------------------------------------------------------
FULL_N = (17, 41, 121)
# eight problems per node count, (seed, k_dur, disc radius as a share of the leg or 0: no disc, corridor half width as a share of the leg,
# 0: no edges, -1: step_corridor's cut of the free plan's bow), chosen on the CPU with the statement alone: it CONVERGES with h strictly
# inside its box, from the 8 starts of nlp_steps_ref.starts (every entry moved by an ulp) it converges to the same cost and h within
# 1e-9 relative -- a hundredth of what the GPU test allows -- and a disc or an edge binds (a dual above 1e-4 = 1e5 mub_min; at 121 nodes
# a binding disc's is 2e-3 .. 5e-3).  tools/dev/nlp_free_fence_select.py prints this table.
FULL_CASES = {17: ((0, 0.0, 0.09, 0.3), (0, 0.5, 0.09, 0.0), (0, 0.0, 0.0, -1), (0, 2.0, 0.07, 0.3), (2, 0.0, 0.0, -1), (2, 2.0, 0.07, 0.3),
                   (3, 0.0, 0.09, 0.3), (3, 0.5, 0.09, 0.0)),
              41: ((0, 0.0, 0.09, 0.3), (0, 0.5, 0.09, 0.0), (0, 2.0, 0.07, 0.3), (1, 0.0, 0.09, 0.3), (1, 0.5, 0.09, 0.0), (1, 0.0, 0.0, -1),
                   (1, 2.0, 0.07, 0.3), (2, 0.0, 0.09, 0.3)),
              121: ((0, 0.0, 0.09, 0.3), (0, 0.5, 0.09, 0.0), (0, 2.0, 0.07, 0.3), (1, 0.0, 0.09, 0.3), (1, 0.5, 0.09, 0.0), (1, 2.0, 0.07, 0.3),
                    (2, 0.0, 0.09, 0.3), (2, 0.5, 0.09, 0.0))}


@functools.lru_cache(maxsize=None)
def full_launch(N):
    """-> list of (FreeProblem, row, W0, discs (MAX_KEEP, 3), edges (MAX_FENCE, 4)) of FULL_CASES[N]"""
    out = []
    for seed, k_dur, Rf, half in FULL_CASES[N]:
        fp, r, W0, discs, edges = detour_problem(N, seed, k_dur, Rf if Rf else 0.09, half if half > 0 else 0.3)
        if half < 0:
            rect = step_corridor(fp, W0, 14.5 * H0 * (N - 1))
            if rect is None:
                raise ValueError(f'full_launch({N}): seed {seed} has no plan without tables to cut a corridor from')
            edges = E.pad(rect)
        out.append((fp, r, W0, discs if Rf else np.zeros((MAX_KEEP, 3)), edges if half else np.zeros((MAX_FENCE, 4))))
    return out


# ---- the independent arbiter: tests/golden/nlp_free_fence_slsqp.npz (tests/golden/make_nlp_free_fence_golden.py) -----------------------
ARB_CASES = ('cut-5', 'cut-9', 'disc-17', 'cut-17', 'mixed-17')


def arbiter_problem(name, k_dur=0.5, h_box=(0.5, 2.0)):
    """A case of the golden file -> FreeProblem, scenario row, W0, discs (n, 3), edges (n, 4).  'disc-N': nlp_keepout_ref.arbiter_problem's
    leg and disc; 'cut-N', 'mixed-N': nlp_fence_ref.arbiter_problem's corridor (and disc).  The step is free in H0 * h_box with the weight
    k_dur on the duration: the leg is laid out for 12 m/s = VSP in (N - 1) H0 seconds, so h ends near H0, strictly inside its box, where
    the duration term balances the speed term; the disc or the edge is active at the optimum (asserted when the golden file is made).
    Tried and dropped: 'disc-5' (the statement converges 1e-9 off in cost after 215 steps with a dual of 492 on a disc whose g is 0.02: too
    stiff an arbiter) and 'disc-9' (SLSQP and the statement pass the disc on different sides: two local minima)."""
    kind, N = name.split('-'); N = int(N)
    if kind == 'disc':
        pb, row, W0, discs = K.arbiter_problem(N, False)
        edges = np.zeros((0, 4))
    else:
        pb, row, W0, discs, edges = E.arbiter_problem(name)
    return F.FreeProblem(pb, H0 * h_box[0], H0 * h_box[1], k_dur), row, W0, np.asarray(discs, float).reshape(-1, 3), np.asarray(edges, float).reshape(-1, 4)
