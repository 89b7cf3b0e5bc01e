"""The cases, the step budgets and the tolerance of the Newton-step-by-Newton-step comparison of the collocation solver with its CPU
statements (tests/test_nlp_steps_cpu.py, tests/test_gpu_nlp_steps.py; test infrastructure only).

A CASE is one statement problem -- a single solve, or one multi-aircraft scenario -- with its start; a LAUNCH is the list of cases
one device call takes, with the arrays that call needs.  Everything is built on the CPU; the device is not touched here.  The
functions that lay out scenario rows import d2dhip for the column constants of include/d2d.h; that package imports without a device
(the library is loaded when a Context is made), as the other CPU tests of the collocation solver rely on.

The tolerance of a case after a budget is measured on the statement alone (measure()): the statement is run from 8 starts in which
every entry of W0 is moved by -1, 0 or +1 ulp (fixed seed), floor = the largest |dW| of its iterate over them, and

    tol = max(1e3 * floor, 64 * eps * max(1, max |W|)).

The factor 1e3 stands for what the kernel does differently at the same conditioning -- fused multiply-adds, lane-order reductions,
block cyclic reduction or the twisted recursion for banded LAPACK, mub * sqrt(mub) for mub ** 1.5: about 25 N more rounding events
than the perturbation injects.
"""
import functools
import zlib

import numpy as np

import nlp_groups_pairs_ref as P
import nlp_groups_wind_ref as G
import nlp_model_ref as MR
import nlp_moving_ref as M
import nlp_wind_ref as R
from oracle import nlp, costs as C

H = 0.1
BUDGETS = ((1, 1), (2, 1), (3, 1), (5, 1), (8, 1), (5, 2), (5, 3), (5, 4))        # (inner_max, outer_max)
N_STARTS = 8
MARGIN = 1e3
TOL_CAP = 1e-8                                  # a case whose tolerance exceeds this is not determined: replace its input
EPS = float(np.finfo(float).eps)
ST_MAXITER = 2


class Case:
    """cid; W0 (1, N, 5) the start; run(W0, inner_max, outer_max) -> W (1, N, 5), info with inner and status (one-element tuples), path
    (the accepted steps in order: length, largest |dW|, eightfold raises of the damping, halvings) and the statement's own info as
    `raw`; fn(W) -> cost, feas of the statement at W."""

    def __init__(self, cid, W0, run, fn=None):
        self.cid, self.W0, self.run, self.fn = cid, np.asarray(W0, float), run, fn

    def __repr__(self):
        return self.cid


class Launch:
    """lid; entry: the Context method; N; cases; kw: what the device call needs beside the cases' starts."""

    def __init__(self, lid, entry, N, cases, **kw):
        self.lid, self.entry, self.N, self.cases, self.kw = lid, entry, N, cases, kw

    def __repr__(self):
        return self.lid


def _scenario(cid, W0s, solve_groups):
    """A multi-aircraft case: solve_groups(W0s, wrap, inner_max, outer_max) -> Ws, infos, sweeps, moved, where wrap(inner) goes round
    the inner solver and collects the paths.  W0 is (n_ac, N, 5); info carries inner and status per aircraft, sweeps and moved."""
    def run(W0, inner_max, outer_max):
        path = []

        def wrap(inner):
            def f(a, pb, W):
                Wn, info = inner(a, pb, W)
                path.extend(info['path'])
                return Wn, info
            return f
        Ws, infos, sweeps, moved = solve_groups([w for w in W0], wrap, inner_max, outer_max)
        return np.stack(Ws), dict(inner=tuple(i['inner'] for i in infos), status=tuple(i['status'] for i in infos), path=tuple(path),
                                  sweeps=sweeps, moved=moved)
    return Case(cid, np.stack(W0s), run)


def _single(cid, W0, solve, fn):
    def run(W0s, inner_max, outer_max):
        W, info = solve(W0s[0], inner_max=inner_max, outer_max=outer_max)
        return W[None], dict(inner=(info['inner'],), status=(info['status'],), path=tuple(info['path']), raw=info)
    return Case(cid, W0[None], run, fn)


# ---- the tolerance ----------------------------------------------------------------------------------------------------------------
def starts(case):
    """The 8 starts of a case: every entry of W0 moved by -1, 0 or +1 ulp."""
    rng = np.random.default_rng(zlib.crc32(case.cid.encode()))
    out = []
    for _ in range(N_STARTS):
        s = rng.integers(-1, 2, case.W0.shape)
        out.append(np.where(s > 0, np.nextafter(case.W0, np.inf), np.where(s < 0, np.nextafter(case.W0, -np.inf), case.W0)))
    return out


_measured = {}


def _lengths_agree(pa, pb):
    """The same discrete decisions step by step (raises of the damping, halvings of the line search) and the same step length.  A
    full step (a power of 1/2: nothing bound it) must be equal exactly.  A length cut by the fraction-to-the-boundary rule is a
    continuous function of the iterate (tau * slack / |dw|), which the perturbation moves by its own floor; there the lengths
    must agree to 1e-9 relative -- what a floor of 1e-11 on a slack of 1e-2 gives.  (The issue asks for identical lengths;
    that cannot be had for a cut length, and this is the departure.)"""
    def same(a, b):
        return a == b if np.log2(b) == np.round(np.log2(b)) else abs(a - b) <= 1e-9 * b
    return len(pa) == len(pb) and all(a[2:] == b[2:] and same(a[0], b[0]) for a, b in zip(pa, pb))


def measure(case, budget):
    """The statement of `case` after `budget`, from its start and from the 8 perturbed ones -> dict(W, info, floor, tol, same_path:
    the step counts and the accepted step lengths are those of the unperturbed run in every perturbed one).  Cached per process."""
    key = (case.cid, budget)
    if key not in _measured:
        W, info = case.run(case.W0, *budget)
        floor, same = 0.0, True
        for W0 in starts(case):
            Wp, ip = case.run(W0, *budget)
            floor = max(floor, float(np.abs(Wp - W).max()))
            same = same and ip['inner'] == info['inner'] and _lengths_agree(ip['path'], info['path'])
        tol = max(MARGIN * floor, 64 * EPS * max(1.0, float(np.abs(W).max())))
        _measured[key] = dict(W=W, info=info, floor=floor, tol=tol, same_path=same)
    return _measured[key]


def check(case, budget):
    """What tests/test_nlp_steps_cpu.py asks of a case after a budget -> list of complaints (empty: the case may be used).
    Determined: tol <= TOL_CAP, and the step counts, the raises of the damping, the halvings and the step lengths are the same from
    all 8 perturbed starts.  Not finished early (budgets with outer_max = 1): every solve ends at 'max iterations', none of them on
    its convergence test or on a step it could not take (each counted step was accepted), and each step moved W by more than
    1e6 tol."""
    m = measure(case, budget)
    info, out = m['info'], []
    if not m['tol'] <= TOL_CAP:
        out.append(f"tol {m['tol']:.1e} > {TOL_CAP:.0e} (floor {m['floor']:.1e})")
    if not m['same_path']:
        out.append('the perturbed starts take another path')
    if budget[1] == 1:
        if any(s != ST_MAXITER for s in info['status']):
            out.append(f"status {info['status']}")
        if len(info['path']) != sum(info['inner']):
            out.append(f"{sum(info['inner'])} steps counted, {len(info['path'])} accepted")
        small = [p[1] for p in info['path'] if not p[1] > 1e6 * m['tol']]
        if small:
            out.append(f"a step moved W by {min(small):.1e} <= 1e6 tol = {1e6 * m['tol']:.1e}")
    return out


def scenario_row(pb, obstacles=(), kobs=0.0, okind=0):
    """d2dhip scenario row of an oracle Problem."""
    import d2dhip as D
    r = np.zeros(D.SCEN_STRIDE)
    r[D.SC_X0:D.SC_X0 + 3] = pb.p0; r[D.SC_X1:D.SC_X1 + 3] = pb.p1
    r[D.SC_VSP], r[D.SC_KV], r[D.SC_KPHI], r[D.SC_S], r[D.SC_KOBS] = pb.vsp, pb.kv, pb.kphi, pb.s, kobs
    r[D.SC_WX], r[D.SC_WY] = -pb.wind[0], -pb.wind[1]
    r[D.SC_PHIMAX] = pb.hi[1, 3]; r[D.SC_VMIN], r[D.SC_VMAX] = pb.lo[1, 4], pb.hi[1, 4]
    if np.isfinite(pb.lo[1, 0]):
        r[D.SC_XMIN], r[D.SC_XMAX] = pb.lo[1, 0], pb.hi[1, 0]
    if np.isfinite(pb.lo[1, 1]):
        r[D.SC_YMIN], r[D.SC_YMAX] = pb.lo[1, 1], pb.hi[1, 1]
    for i, o in enumerate(obstacles):
        c = D.obs_col(i)
        r[c:c + 3] = o
    r[D.SC_OKIND] = okind
    return r


# ---- single solves ----------------------------------------------------------------------------------------------------------------
def _start(p0, p1, N, seed):
    """A start that is far from a plan: the straight line with a lateral bow of 8 % of the leg, headings, bank angles and speeds that
    swing, and noise of 1 % on everything."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, N)
    d = np.array(p1[:2]) - np.array(p0[:2]); L = float(np.hypot(*d)); nrm = np.array([-d[1], d[0]]) / L
    W = np.zeros((N, 5))
    W[:, :2] = np.array(p0[:2]) + t[:, None] * d + (0.08 * L * np.sin(np.pi * t))[:, None] * nrm
    W[:, 2] = p0[2] + t * (p1[2] - p0[2]) + 0.3 * np.sin(2 * np.pi * t)
    W[:, 3] = 0.2 * np.cos(3.0 * t)
    W[:, 4] = 11.0 + np.sin(4.0 * t)
    return W + 0.01 * rng.standard_normal(W.shape) * np.array([L / 10, L / 10, 1.0, 1.0, 1.0])


# seed of every other case by its id, chosen in the same way (not listed: 0)
SEEDS = {'wind-vortex-41': 1, 'wind-shear-122': 2, 'wind-gust-122': 2, 'moving-const-crossing-kind1': 1, 'moving-const-headon-kind1': 1,
         'model-41-1-partial': 22, 'model-65-1-partial': 7,
         'groups-3-sweeps1-pair': 3, 'groups-3-sweeps2-pair': 2, 'groupswind-2-sweeps1-pair': 2, 'groupswind-2-sweeps2-pair': 3,
         'pairsconst-3-sweeps1-pair': 3, 'pairsconst-3-sweeps1-all': 1, 'pairsconst-3-sweeps2-pair': 2,
         'pairsconst-3-sweeps2-chain': 18, 'pairsconst-3-sweeps2-all': 12, 'pairsfield-3-sweeps2-chain': 23,
         'groupsmoving-3-sweeps2-chain': 24, 'groupsmoving-3-sweeps2-all': 12,
         'pairsfield-2-sweeps1-pair': 2, 'pairsfield-2-sweeps2-pair': 3, 'pairsfield-3-sweeps1-chain': 5, 'pairsfield-3-sweeps1-all': 5,
         'groupsmoving-2-sweeps1-pair': 1, 'groupsmoving-3-sweeps1-pair': 3, 'groupsmoving-3-sweeps1-all': 1, 'groupsmoving-3-sweeps2-pair': 2}
PLAIN_TAGS = ('disc1', 'disc0', 'windbox', 'bankmax')
# seed of each plain case: the first one, counted from 0, at which the statement is determined and keeps stepping after every budget
# (check() below; found on the CPU with the statement alone).  Cases that are not listed use seed 0.
PLAIN_SEEDS = {(3, 'disc1'): 3, (3, 'windbox'): 4, (5, 'disc1'): 5, (5, 'bankmax'): 1, (64, 'disc1'): 2, (64, 'disc0'): 1, (65, 'disc0'): 2,
               (65, 'bankmax'): 1, (121, 'disc1'): 3, (121, 'disc0'): 1, (129, 'bankmax'): 1}


def plain_case(N, tag, seed):
    """One row of plain_launch -> case, scenario row."""
    import d2dhip as D
    L = 11.5 * H * (N - 1)
    rng = np.random.default_rng([N, PLAIN_TAGS.index(tag), seed])
    p0 = (0.0, 0.0, rng.uniform(-0.3, 0.3)); p1 = (L * rng.uniform(0.93, 1.0), 0.12 * L * rng.uniform(-1, 1), rng.uniform(-0.3, 0.3))
    # (a cost of order ten: the inner tolerance of the first look is 0.1 ABSOLUTE, and a small problem with a small cost meets it in
    # fewer than 8 steps)
    kw = dict(vsp=12.0, kv=5.0, kphi=1.0, obj_scale=10.0 * N if N <= 5 else float(N) / 4, phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0)
    ob, kind = [], 1
    if tag == 'disc1':
        ob = [(0.5 * p1[0] + 0.02 * L, 0.5 * p1[1] - 0.03 * L, max(0.12 * L, 0.5))]
    if tag == 'disc0':                           # r^2 - d^2 > log 1e3 on the nodes near the middle of the start: inside the clip
        ob, kind = [(0.5 * p1[0] + 0.02 * L, 0.5 * p1[1] + 0.08 * L, max(0.1 * L, 3.2))], 0
    if tag == 'windbox':                         # the bow of the start is outside the box: the start is pushed inside
        kw.update(wind=(1.0, -0.5), y_box=(min(0.0, p1[1]) - 0.01 * L, max(0.0, p1[1]) + 0.01 * L))
    if tag == 'bankmax':
        kw.update(bank_max=True)
    kobs = 0.0 if not ob else 20.0 if (N <= 5 and kind == 1) else 1.0      # (a short leg: a disc that weighs as much as the speed term)
    pb = nlp.Problem(N, H, p0, p1, obstacles=ob, kobs=kobs, obs_kind=kind, **kw)
    r = scenario_row(pb, ob, kobs, 1 if (ob and kind == 0) else 0)
    r[D.SC_BANKMAX] = 1.0 if tag == 'bankmax' else 0.0
    W0 = _start(p0, p1, N, rng.integers(1 << 30))
    if tag == 'disc0':
        arg = ob[0][2] ** 2 - (W0[:, 0] - ob[0][0]) ** 2 - (W0[:, 1] - ob[0][1]) ** 2
        assert (arg[1:-1] > nlp.LOG_CLIP).any()
    if tag == 'windbox':
        assert (W0[1:-1, 1] < pb.lo[1, 1]).any() or (W0[1:-1, 1] > pb.hi[1, 1]).any()
    case = _single(f'plain-{N}-{tag}', W0, functools.partial(nlp.solve, pb),
                   lambda W: (nlp.cost(pb, W), float(np.abs(nlp.constraints(pb, W)).max())))
    return case, r


def plain_launch(N):
    """d2d_nlp_solve, one ragged launch: a kind-1 disc, a kind-0 disc whose clip holds the start, constant wind with a y box that
    holds the start's bow out, and a CostBank max-mode row (its budgets are three times as long on both sides:
    D2D_NLP_BANKMAX_BATCHES)."""
    cr = [plain_case(N, tag, PLAIN_SEEDS.get((N, tag), 0)) for tag in PLAIN_TAGS]
    return Launch(f'plain-{N}', 'nlp_solve', N, [c for c, _ in cr], rows=np.stack([r for _, r in cr]))


def bounds_launch():
    """d2d_nlp_solve with d2d_nlp_opts.bounds: a left turn with phi in [-5, +35] deg and psi in [-0.2, 2.0] against the same row
    without an override."""
    N = 41
    p0 = (0.0, 0.0, 0.0, 0.0, 12.0); p1 = (26.0, 32.0, 1.8, 0.0, 12.0)
    mk = lambda: nlp.Problem(N, H, p0, p1, vsp=12.0, kv=1.0, kphi=0.5, obj_scale=1.0, phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0)
    pa, pb = mk(), mk()
    bnd = (-np.deg2rad(5.0), np.deg2rad(35.0), -0.2, 2.0)
    pa.lo[:, 3], pa.hi[:, 3] = bnd[0], bnd[1]
    pa.lo[1:-1, 2], pa.hi[1:-1, 2] = bnd[2], bnd[3]
    W0 = nlp.from_free(C.single_guess('tri', p0, p1, 12.0, (N - 1) * H, N), N)
    cases = [_single(f'bounds-{tag}', W0, functools.partial(nlp.solve, p), lambda W, p=p: (nlp.cost(p, W), float(np.abs(nlp.constraints(p, W)).max())))
             for tag, p in (('interval', pa), ('row', pb))]
    return Launch('bounds-41', 'nlp_solve', N, cases, rows=np.stack([scenario_row(pb), scenario_row(pb)]), bounds=np.array([bnd, (0.0, 0.0, 0.0, 0.0)]))


T_START_GUST = 3.0


def wind_launch(N, name):
    """d2d_nlp_solve_wind in a field of nlp_wind_ref.fields(): a leg like those of nlp_wind_ref.field_problems(41, .) scaled to N
    nodes (11.5 m/s over the ground) round a kind-1 disc, from the 'tri' guess; the unsteady gust starts at T_START_GUST."""
    import d2dhip as D
    F = R.fields()[name]
    t_start = T_START_GUST if name == 'gust' else 0.0
    cid = f'wind-{name}-{N}'
    rng = np.random.default_rng([N, SEEDS.get(cid, 0)])
    L = 11.5 * H * (N - 1)
    p0 = (0.0, 0.0, rng.uniform(-0.5, 0.5), 0.0, 12.0); p1 = (L + rng.uniform(-3, 3), rng.uniform(-6, 6), rng.uniform(-0.4, 0.4), 0.0, 12.0)
    ob = [(0.5 * L + rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 6))]
    pb = nlp.Problem(N, H, p0, p1, vsp=12.0, kv=5.0, kphi=1.0, obj_scale=1.0, phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0,
                     obstacles=ob, kobs=1.0, obs_kind=1)
    fp = R.FieldProblem(pb, F, t_start)
    r = scenario_row(pb, ob, 1.0, 0)
    r[D.SC_WX] = r[D.SC_WY] = np.nan               # not read in a field
    W0 = nlp.from_free(C.single_guess('tri', p0, p1, 12.0, (N - 1) * H, N), N)
    case = _single(cid, W0, functools.partial(R.solve, fp), lambda W: (nlp.cost(pb, W), float(np.abs(R.constraints(fp, W)).max())))
    return Launch(cid, 'nlp_solve_wind', N, [case], rows=r[None], field=name, t_start=t_start)


MOVING_WIND = (1.0, -0.5)


def moving_launch(wind):
    """d2d_nlp_solve_moving, N = 61: the crossing and the head-on disc of nlp_moving_ref's catalogue, kind 1 and kind 0, in a constant
    wind or in the gust; the kind-0 problems start 1.5 s after the kind-1 ones (every track is anchored at its problem's start time)."""
    N = M.N_NODES
    F = None if wind == 'const' else R.fields()['gust']
    leg = M.LEG if wind == 'const' else M.LEG_GUST
    t0s = {1: 0.0, 0: 1.5} if wind == 'const' else {1: M.GUST_T_START, 0: M.GUST_T_START + 1.5}
    cases, rows, moving, ts = [], [], [], []
    for kind in (1, 0):
        for name in ('crossing', 'headon'):
            r = M.row(kind, p1=(leg, 0.0, 0.0), wind=MOVING_WIND if wind == 'const' else (0.0, 0.0))
            mv = M.catalogue(kind, t0s[kind], leg)[name]
            pb = M.problem(r, mv, t0s[kind])
            if F is None:
                solve = functools.partial(nlp.solve, pb)
                fn = lambda W, pb=pb: (nlp.cost(pb, W), float(np.abs(nlp.constraints(pb, W)).max()))
            else:
                fp = R.FieldProblem(pb, F, t0s[kind])
                solve = functools.partial(R.solve, fp)
                fn = lambda W, fp=fp: (nlp.cost(fp.pb, W), float(np.abs(R.constraints(fp, W)).max()))
            cid = f'moving-{wind}-{name}-kind{kind}'
            seed = SEEDS.get(cid, 0)      # the straight line (seed 0), or a bowed start where the statement is done too soon from it
            W0 = M.straight_guess(r) if seed == 0 else _start(r[:3], (leg, 0.0, 0.0), N, seed)
            cases.append(_single(cid, W0, solve, fn))
            rows.append(r); moving.append(mv); ts.append(t0s[kind])
    return Launch(f'moving-{wind}', 'nlp_solve_moving', N, cases, rows=np.stack(rows), moving=moving, field=None if F is None else 'gust',
                  t_start=np.array(ts))


# ---- the quadratic model -----------------------------------------------------------------------------------------------------------
def _spd_blocks(rng, N, scale):
    """Random symmetric positive-definite 5x5 blocks, condition <= 1e3, all 15 planes distinct and non-zero."""
    H5 = np.zeros((N, 5, 5))
    for i in range(N):
        Q, _ = np.linalg.qr(rng.standard_normal((5, 5)))
        ev = scale * 10.0 ** rng.uniform(-1.5, 1.4, 5)
        H5[i] = (Q * ev) @ Q.T
        H5[i] = 0.5 * (H5[i] + H5[i].T)
    planes = MR.pack(H5)
    assert np.linalg.cond(H5).max() <= 1e3 and (planes != 0.0).all()
    assert all(not np.array_equal(planes[a], planes[b]) for a in range(15) for b in range(a + 1, 15))
    return H5


def model_problem(N, kind, seed):
    """One d2d_nlp_solve_model problem: the row (structured terms zero), the model (g, H, Wc) and a start that is not Wc.
    kind: 'spd', 'partial' (non-zero on the (x, y) sub-block only, zero blocks on every third node) or 'indefinite' (the SPD model
    with a mildly indefinite block on a few nodes)."""
    rng = np.random.default_rng(seed)
    L = 11.5 * H * (N - 1)
    p0 = (0.0, 0.0, rng.uniform(-0.2, 0.2)); p1 = (L * rng.uniform(0.95, 1.0), 0.1 * L * rng.uniform(-1, 1), rng.uniform(-0.2, 0.2))
    pb = nlp.Problem(N, H, p0, p1, vsp=12.0, kv=0.0, kphi=0.0, obj_scale=1.0, phi_max=np.deg2rad(35.0), v_min=9.0, v_max=15.0,
                     wind=(0.5, -0.3))
    t = np.linspace(0.0, 1.0, N)
    Wc = np.stack([p0[0] + t * (p1[0] - p0[0]), p0[1] + t * (p1[1] - p0[1]), p0[2] + t * (p1[2] - p0[2]), np.zeros(N), np.full(N, 11.5)], 1)
    Wc += rng.standard_normal(Wc.shape) * np.array([0.02 * L, 0.02 * L, 0.05, 0.05, 0.3])
    g = rng.standard_normal((N, 5)) * np.array([0.3, 0.3, 1.0, 1.0, 0.5])
    if kind == 'partial':
        H5 = np.zeros((N, 5, 5))
        H5[:, :2, :2] = _spd_blocks(rng, N, 1.0)[:, :2, :2]
        H5[::3] = 0.0
        g[:, 2:] = 0.0
    else:
        H5 = _spd_blocks(rng, N, 1.0)
        if kind == 'indefinite':                 # a negative curvature of -2 along (psi, phi, v) on three interior nodes
            for i in (N // 4, N // 2, N // 2 + 1):
                u = np.array([0.0, 0.0, 0.6, 0.6, 0.529150262212918])
                H5[i] = H5[i] - (u @ H5[i] @ u + 2.0) * np.outer(u, u)
                H5[i] = 0.5 * (H5[i] + H5[i].T)
                assert np.linalg.eigvalsh(H5[i]).min() < -0.5
    mp = MR.ModelProblem(pb, g, H5, Wc)
    return mp, scenario_row(pb), _start(p0, p1, N, seed + 7)


def model_launch(N):
    """d2d_nlp_solve_model, B = 3 with a different model per problem: SPD, partial, SPD again (another seed)."""
    cases, rows, mps = [], [], []
    for b, kind in enumerate(('spd', 'partial', 'spd')):
        cid = f'model-{N}-{b}-{kind}'
        mp, r, W0 = model_problem(N, kind, 500 + 10 * N + b + 1000 * SEEDS.get(cid, 0))
        cases.append(_single(cid, W0, functools.partial(MR.solve, mp),
                             lambda W, mp=mp: (mp.value(W), float(np.abs(mp.constraints(W)).max()))))
        rows.append(r); mps.append(mp)
    return Launch(f'model-{N}', 'nlp_solve_model', N, cases, rows=np.stack(rows), models=mps)


def indefinite_launch():
    N = 41
    mp, r, W0 = model_problem(N, 'indefinite', 77)
    case = _single('model-41-indefinite', W0, functools.partial(MR.solve, mp), lambda W: (mp.value(W), float(np.abs(mp.constraints(W)).max())))
    return Launch('model-indefinite-41', 'nlp_solve_model', N, [case], rows=r[None], models=[mp])


def full_model_launch():
    """One full solve per model at 41 nodes (SPD, partial, indefinite; seeds at which the statement converges in 47 .. 59 steps with
    a KKT residual <= 1.1e-7 -- other SPD seeds need 1400 .. 2300 steps, which is no test of a few seconds)."""
    cases, rows, mps = [], [], []
    for kind, seed in (('spd', 21), ('partial', 4911), ('indefinite', 77)):
        mp, r, W0 = model_problem(41, kind, seed)
        cases.append(_single(f'model-full-{kind}', W0, functools.partial(MR.solve, mp), lambda W, mp=mp: (mp.value(W), float(np.abs(mp.constraints(W)).max()))))
        rows.append(r); mps.append(mp)
    return Launch('model-full-41', 'nlp_solve_model', 41, cases, rows=np.stack(rows), models=mps)


# ---- multi-aircraft scenarios ------------------------------------------------------------------------------------------------------
GROUP_N = 41
GROUP_FIELD = 'shear'
GROUP_ENTRIES = ('groups', 'groupswind', 'pairsconst', 'pairsfield', 'groupsmoving')
GROUP_METHOD = {'groups': 'nlp_solve_groups', 'groupswind': 'nlp_solve_groups_wind', 'pairsconst': 'nlp_solve_groups_pairs',
                'pairsfield': 'nlp_solve_groups_pairs', 'groupsmoving': 'nlp_solve_groups_moving'}
MASKS = {2: {'pair': [(0, 1)]}, 3: {'pair': [(0, 1)], 'chain': [(0, 1), (1, 2)], 'all': [(0, 1), (0, 2), (1, 2)]}}
GROUP_T_START = 2.5


def group_case(entry, n_ac, name, max_sweeps, k=0):
    """One scenario of a groups entry point at 41 nodes: nlp_groups_pairs_ref.crossing for n_ac aircraft on legs of 4 s (9 m/s over
    the ground in CONST_WIND, 8 m/s against the field), the tracks 6 .. 8 m apart where they cross (inside rcol = 10 m), from the
    'tri' guesses; `name` the partner sets of MASKS (the two pair entries take the pair (0, 1) from the collision columns);
    groupsmoving: a kind-1 disc of 5 m crosses the tracks from the south.  Every solve of the alternation carries the step budget.
    -> case, rows, discs or None, start time."""
    import d2dhip as D
    N = GROUP_N
    cid = f'{entry}-{n_ac}-sweeps{max_sweeps}-{name}'
    rng = np.random.default_rng([n_ac, SEEDS.get(cid, 0)])
    F = R.fields()[GROUP_FIELD] if entry in ('groupswind', 'pairsfield') else None
    leg = 32.0 if F is not None else 36.0
    th = np.array([0.0, 0.25, -0.15])[:n_ac] + rng.uniform(-0.03, 0.03, n_ac)
    off = np.array([0.0, 7.0, -6.5])[:n_ac] + rng.uniform(-1.0, 1.0, n_ac)
    p0s, p1s = P.crossing((-13.0 + rng.uniform(-3, 3), rng.uniform(-3, 3)), leg, th, off)
    wind = (0.0, 0.0) if F is not None else P.CONST_WIND
    t0 = GROUP_T_START + 0.7 * k
    rows = G.group_rows(p0s, p1s, wind) if entry in ('groups', 'groupswind') else P.pair_rows(p0s, p1s, MASKS[n_ac][name], wind)
    W0s = []
    for r in rows:
        p0 = tuple(r[D.SC_X0:D.SC_X0 + 3]) + (0.0, 12.0); p1 = tuple(r[D.SC_X1:D.SC_X1 + 3]) + (0.0, 12.0)
        W0s.append(nlp.from_free(C.single_guess('tri', p0, p1, 12.0, (N - 1) * H, N), N))
    mv = None
    if entry == 'groupsmoving':
        rows[:, D.SC_KOBS] = M.GROUP_KOBS
        mv = [M.MovingObstacle.linear((-13.0, -20.0), (0.0, 8.0), 5.0, t0=t0, t1=t0 + M.T_END)]

    def solve_groups(W0, wrap, inner_max, outer_max):
        pbs = [nlp.problem_from_row(r, N, H) for r in rows]
        if mv is not None:
            pbs = [M.with_moving(pb, mv, t0) for pb in pbs]
        inner = wrap(P.in_field(F, t0, inner_max=inner_max, outer_max=outer_max) if F is not None
                     else P.in_constant_wind(inner_max=inner_max, outer_max=outer_max))
        if entry in ('groups', 'groupswind'):
            return G.solve_groups(pbs, W0, inner, max_sweeps=max_sweeps)
        return P.solve_groups(pbs, W0, inner, P.masks_of(rows), max_sweeps=max_sweeps)
    return _scenario(cid, W0s, solve_groups), rows, mv, t0


def group_launch(entry, n_ac, max_sweeps, part=None):
    """One launch of a groups entry point: one scenario per partner-set name (the two pair entries: the default pair alone).  With
    three aircraft the three partner sets would be nine solves in a launch; no launch is to hold more than eight, so they go in two
    parts: 'pc' (one pair, the chain) and 'all'."""
    every = list(MASKS[n_ac])
    names = ['pair'] if entry in ('groups', 'groupswind') else every if part is None else ['pair', 'chain'] if part == 'pc' else ['all']
    got = [group_case(entry, n_ac, name, max_sweeps, every.index(name)) for name in names]
    return Launch(f'{entry}-{n_ac}-sweeps{max_sweeps}' + (f'-{part}' if part else ''), GROUP_METHOD[entry], GROUP_N, [g[0] for g in got], rows=np.concatenate([g[1] for g in got]),
                  n_ac=n_ac, max_sweeps=max_sweeps, field=GROUP_FIELD if entry in ('groupswind', 'pairsfield') else None,
                  t_start=np.array([g[3] for g in got]), moving=[g[2] for g in got] if entry == 'groupsmoving' else None)


PLAIN_N = (3, 5, 64, 65, 121, 122, 129)
WIND_N = (41, 65, 122)
MODEL_N = (5, 41, 65)


@functools.lru_cache(maxsize=None)
def launch(lid):
    """The launch of an id of launch_ids() (built once per process: the cases carry the cache keys of measure())."""
    k = lid.split('-')
    if k[0] == 'plain':
        return plain_launch(int(k[1]))
    if k[0] == 'bounds':
        return bounds_launch()
    if k[0] == 'wind':
        return wind_launch(int(k[2]), k[1])
    if k[0] == 'moving':
        return moving_launch(k[1])
    if k[0] == 'model':
        return indefinite_launch() if k[1] == 'indefinite' else model_launch(int(k[1]))
    return group_launch(k[0], int(k[1]), int(k[2][len('sweeps'):]), k[3] if len(k) > 3 else None)


def group_launch_ids():
    return [f'{e}-{n}-sweeps{sw}{part}' for e in GROUP_ENTRIES for n in (2, 3) for sw in (1, 2)
            for part in (('-pc', '-all') if n == 3 and e not in ('groups', 'groupswind') else ('',))]


def launch_ids():
    return ([f'plain-{N}' for N in PLAIN_N] + ['bounds-41'] + [f'wind-{f}-{N}' for N in WIND_N for f in ('shear', 'vortex', 'gust')]
            + ['moving-const', 'moving-gust'] + [f'model-{N}' for N in MODEL_N] + ['model-indefinite-41']
            + group_launch_ids())
