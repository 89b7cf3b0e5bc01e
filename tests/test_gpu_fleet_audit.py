"""GPU parity of the fleet audit (d2d_fleet_audit, csrc/fleet_audit.hip) with its CPU statement tests/fleet_audit_ref.py (brute force
over all pairs): small synthetic histories, the bit-identity of every output across the scheduling knobs, pairs placed on the grid's
cell edges, the look radius, ties, worlds, refusals, D2D_EINVAL, its bit-identity with the in-formation audit, and a flown history.

Tolerances, as in test_gpu_flight_audit.py: distances 1e-10 m absolute; partners, counts and status equal, on inputs the CPU statement
shows to be 1e-6 m away from every decision (look radius, d_safe, partner choice, step bound); a reported time gives the reported
minimum within 1e-10 when the statement's distance function is evaluated there, and equals the statement's time within 1e-9 dt_row
where the relative motion of that segment is >= 1 m."""
import ctypes as C

import numpy as np
import pytest

import fleet_audit_ref as FL
import flight_audit_ref as FA

pytestmark = pytest.mark.gpu
TOL = 1e-10
KEYS = ('near_dist', 'near_partner', 'near_time', 'near_count', 'status')
STEP = 4.3          # synthetic_history moves up to 3 m per row and axis: 3 sqrt 2 = 4.243


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    return d2dhip.default_context()


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _run(ctx, X, n_ac, dt, d_look, step_max, **kw):
    import torch
    dev = dict(kw)
    for k in ('rows', 'row0', 'world'):
        if dev.get(k) is not None:
            dev[k] = torch.as_tensor(np.ascontiguousarray(dev[k]), dtype=torch.int32).to(ctx.device)
    out = ctx.fleet_audit(ctx.dev(np.ascontiguousarray(X)), n_ac, dt, d_look, step_max, **dev)
    ctx.sync()
    return _np(out)


def _same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in KEYS)


def _compare(got, X, n_ac, dt, d_look, step_max, what='', check_margins=True, **kw):
    """The device's dictionary against the CPU statement on the same inputs."""
    kw = {k: v for k, v in kw.items() if k not in ('tile_rows', 'slots')}
    mg = {}
    ref = FL.audit(X, n_ac, dt, d_look, step_max, margins=mg, **kw)
    assert not check_margins or min(mg.values()) > 1e-6, (what, mg)       # no decision within 1e-6 m of turning
    for k in ('status', 'near_partner', 'near_count'):
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    fin = np.isfinite(ref['near_dist'])
    assert np.array_equal(got['near_dist'][~fin], ref['near_dist'][~fin], equal_nan=True), what
    assert float(np.abs(got['near_dist'][fin] - ref['near_dist'][fin]).max(initial=0.0)) <= TOL, what
    assert np.array_equal(np.isnan(got['near_time']), np.isnan(ref['near_time'])), what
    n_form = X.shape[2] // n_ac
    row0 = np.zeros(n_form, int) if kw.get('row0') is None else np.asarray(kw['row0'])
    for d in np.nonzero(~np.isnan(ref['near_time']))[0]:
        e, t, tr = int(got['near_partner'][d]), got['near_time'][d], ref['near_time'][d]
        assert abs(FL.pair_distance(X, dt, d, e, t, row0[d // n_ac], row0[e // n_ac]) - got['near_dist'][d]) <= TOL, (what, d)
        g = int(np.floor(tr / dt + 1e-9))
        i, ie = g - row0[d // n_ac], g - row0[e // n_ac]
        if tr / dt - g > 1e-9 and np.hypot(*((X[ie + 1, :2, e] - X[i + 1, :2, d]) - (X[ie, :2, e] - X[i, :2, d]))) >= 1.0:
            assert abs(t - tr) <= 1e-9 * dt, (what, d, t, tr)      # s* is well conditioned
        elif tr / dt - g <= 1e-9:
            assert abs(t - tr) <= 1e-9 * dt, (what, d, t, tr)      # a row's own candidate: the row's time
    return ref


def parity_case(n_form, n_ac, n_rows):
    """The history of a parity case, dense enough that most aircraft see another formation within d_look = 25 m, and its clocks."""
    N = n_form * n_ac
    seed = 1000 * n_form + 10 * n_ac + n_rows
    X = FA.synthetic_history(n_form, n_ac, n_rows, seed, span=max(8.0, 6.0 * np.sqrt(N)))
    rng = np.random.default_rng(seed + 1)
    rows = rng.integers(0, n_rows + 1, n_form)
    rows[:3] = [n_rows, 1, 0][:min(3, n_form)]
    row0 = rng.integers(0, n_rows // 2 + 2, n_form)               # overlaps and gaps
    row0[:2] = [0, min(1, n_rows - 1)][:min(2, n_form)]          # the formation of one row meets the first one
    world = (np.arange(n_form) // 2) % (2 if n_form < 9 else 3)
    Xn = X.copy()
    for f in range(n_form):
        Xn[rows[f]:, :, f * n_ac:(f + 1) * n_ac] = np.nan
    return X, Xn, dict(rows=rows, row0=row0, world=world, d_safe=12.0)


SHAPES = [(1, 1), (2, 1), (3, 3), (13, 5), (2, 64), (70, 1), (22, 3)]


@pytest.mark.parametrize('n_rows', [1, 2, 3, 33])
@pytest.mark.parametrize('n_form,n_ac', SHAPES)
def test_parity_with_the_cpu_statement(ctx, n_form, n_ac, n_rows):
    dt, look = 0.5, 25.0
    X, Xn, kw = parity_case(n_form, n_ac, n_rows)
    ref = _compare(_run(ctx, X, n_ac, dt, look, STEP, d_safe=12.0), X, n_ac, dt, look, STEP, 'bare', d_safe=12.0)
    if n_form > 1:
        assert np.isfinite(ref['near_dist']).mean() > 0.5        # most aircraft see someone: the test is not vacuous
    else:
        assert (ref['near_partner'] == -1).all()
    got = _run(ctx, Xn, n_ac, dt, look, STEP, **kw)
    assert (got['status'] == 0).all()                # a refusal here: a row behind rows[f] was read
    ref = _compare(got, Xn, n_ac, dt, look, STEP, 'clocks', **kw)
    if n_form >= 13 and n_rows >= 3:
        assert np.isfinite(ref['near_dist']).any() and (ref['near_partner'] == -1).any()


def test_the_grid_only_schedules(ctx):
    """tile_rows and slots change which pairs are looked at and when, and no bit of any output; slots = 1 is brute force on the device."""
    n_form, n_ac, n_rows, dt = 11, 3, 14, 0.5
    _, Xn, kw = parity_case(n_form, n_ac, n_rows)
    g_rows = int((kw['row0'] + kw['rows']).max())
    first = _run(ctx, Xn, n_ac, dt, 25.0, STEP, **kw)
    _compare(first, Xn, n_ac, dt, 25.0, STEP, 'schedule', **kw)
    assert np.isfinite(first['near_dist']).any()
    for tile in (0, 1, 2, 7, n_rows, g_rows):
        for slots in (0, 1, 2, 64):
            assert _same_bytes(_run(ctx, Xn, n_ac, dt, 25.0, STEP, tile_rows=tile, slots=slots, **kw), first), (tile, slots)
    assert _same_bytes(_run(ctx, Xn, n_ac, dt, 25.0, STEP, **kw), first)          # and from call to call


LOOK_E, STEP_E = 10.0, 3.0
EDGE = (LOOK_E + 2.0 * STEP_E) * (1.0 + FL.EDGE_MARGIN)
ORIGINS = [(0.0, 0.0), (-30.0 * EDGE, 20.0 * EDGE), (-4001.0 * EDGE, -377.0 * EDGE), (62500.0 * EDGE, -62499.0 * EDGE)]      # cell corners; the last: |x|, |y| = 1e6 m
APART = 31.0 * EDGE         # between two pairs: whole cells, about 500 m


def edge_pairs():
    """Pairs of single-aircraft formations, two rows each, around the corners of grid cells: head-on, closing at step_max each from
    just under d_look + 2 step_max apart, so that row 1 is just inside d_look (s = 1: the next row's own candidate -- the only way
    to come from that far, see near_miss_pairs).  At row 0 the two are in cells that differ along x, along y or along both, one of
    them 0.01 m from the corner.  Returns X [2][5][N]."""
    P = []
    gap = LOOK_E + 2.0 * STEP_E - 1e-3
    for ox, oy in ORIGINS:
        k = 0
        for ux, uy in ((1.0, 0.0), (0.0, 1.0), (0.6, 0.8), (-0.8, 0.6)):
            for back in (0.01, gap - 0.01):
                cx, cy = ox + APART * k, oy
                k += 1
                a0 = np.array([cx - back * ux, cy - back * uy])      # A this far behind the corner, B on the other side of it
                b0 = a0 + gap * np.array([ux, uy])
                u = np.array([ux, uy])
                P.append((a0, a0 + STEP_E * u * (1 - 1e-5)))
                P.append((b0, b0 - STEP_E * u * (1 - 1e-5)))
    X = np.zeros((2, 5, len(P)))
    for d, (p0, p1) in enumerate(P):
        X[0, :2, d], X[1, :2, d] = p0, p1
    return X


LOOK_T = 1.0
EDGE_T = (LOOK_T + 2.0 * STEP_E) * (1.0 + FL.EDGE_MARGIN)        # 7.0001 m: the grid of the tests that run with d_look = 1 m
# corners of that grid, at multiples of four cells (so also corners of a grid of edge d_look + step_max = 4 m); the last: 1e6 m
ORIGINS_T = [(0.0, 0.0), (-12.0 * EDGE_T, 8.0 * EDGE_T), (-4000.0 * EDGE_T, -376.0 * EDGE_T), (142856.0 * EDGE_T, -142856.0 * EDGE_T)]
APART_T = 72.0 * EDGE_T       # between two pairs: whole cells, about 500 m


def cells(P, edge):
    """The grid cell of positions [..., 2] for a cell edge, by the library's expression."""
    return np.floor(np.asarray(P) * (1.0 / edge)).astype(np.int64)


def tunnel_pairs():
    """Crossing pairs whose only point below d_look = 1 m is inside the segment 1 -> 2: at right angles past a corner of the grid of
    d_look = 1 m, about half a step from it at either row.  Three rows."""
    P = []
    for ox, oy in ORIGINS_T:
        for k, (h, w) in enumerate(((0.5, 0.02), (0.375, 0.25), (0.625, -0.125))):
            cx, cy = ox + APART_T * k, oy + APART_T
            i = np.arange(3) - 1.0 - h                           # the corner is passed at row 1 + h
            P.append(np.stack([cx + STEP_E * i * 0.99, np.full(3, cy + w)], 1))
            P.append(np.stack([np.full(3, cx + 0.02), cy + STEP_E * i * 0.99], 1))
    X = np.zeros((3, 5, len(P)))
    for d, p in enumerate(P):
        X[:, :2, d] = p
    return X


def near_miss_pairs():
    """What pins the step term of the cell edge.  An interior closest approach q is perpendicular to the relative motion d, so
    |p0|^2 = |q|^2 + s*^2 |d|^2 < d_look^2 + 4 step_max^2: pairs that pass 0.99 m abeam (d_look = 1 m) at s* = 0.97, closing at
    step_max each, start 5.9 m apart -- as far as an interior candidate can start (6.08 m) -- and are 1.006 m apart at row 1, so that
    the interior point is the ONLY candidate below d_look.  They are placed around cell corners so that at row 0 they sit in
    different cells (along x, along y, diagonally) and, under an edge of d_look + step_max, in cells that are not neighbours.
    Two rows.  Returns X [2][5][N]."""
    P = []
    sp, s_star, w = STEP_E * (1 - 1e-5), 0.97, 0.99
    for ox, oy in ORIGINS_T:
        for k, (ux, uy) in enumerate(((1.0, 0.0), (0.0, 1.0), (0.6, 0.8), (-0.8, 0.6))):
            c = np.array([ox + APART_T * k, oy - APART_T])
            u, n = np.array([ux, uy]), np.array([-uy, ux])
            p0 = s_star * 2.0 * sp * u + w * n                   # B - A at row 0
            a0 = c + np.where(np.abs(p0) > 2.0, -0.5 * np.sign(p0), 2.0)       # across the corner along the large components only
            P.append((a0, a0 + sp * u))
            P.append((a0 + p0, a0 + p0 - sp * u))
    X = np.zeros((2, 5, len(P)))
    for d, (q0, q1) in enumerate(P):
        X[0, :2, d], X[1, :2, d] = q0, q1
    return X


def test_cell_edges_closing_pairs(ctx):
    X = edge_pairs()
    N = X.shape[2]
    got = _run(ctx, X, 1, 0.5, LOOK_E, STEP_E)
    _compare(got, X, 1, 0.5, LOOK_E, STEP_E, 'closing')
    assert np.array_equal(got['near_partner'], np.arange(N) ^ 1)                  # every pair found
    assert np.abs(got['near_dist'] - (LOOK_E - 1e-3)).max() <= 1e-4 and (got['near_time'] == 0.5).all()
    assert _same_bytes(_run(ctx, X, 1, 0.5, LOOK_E, STEP_E, slots=1), got)


def test_cell_edges_tunnelling_pairs(ctx):
    X = tunnel_pairs()
    N = X.shape[2]
    look = LOOK_T
    assert np.hypot(X[:, 0, 0::2] - X[:, 0, 1::2], X[:, 1, 0::2] - X[:, 1, 1::2]).min() > look + 0.5        # no row sees it
    diff = cells(X[1, :2, 0::2].T, EDGE_T) - cells(X[1, :2, 1::2].T, EDGE_T)       # at the first row of the crossing segment
    assert (np.abs(diff).max(axis=1) == 1).all() and (np.abs(diff).sum(axis=1) == 2).sum() >= 8      # never one cell; diagonal for w > 0
    got = _run(ctx, X, 1, 0.5, look, STEP_E, d_safe=1.0)
    ref = _compare(got, X, 1, 0.5, look, STEP_E, 'tunnel', d_safe=1.0)
    assert np.array_equal(got['near_partner'], np.arange(N) ^ 1) and (got['near_dist'] < 0.3).all() and (got['near_count'] == 0).all()
    assert np.abs(got['near_time'] - ref['near_time']).max() <= 1e-9 * 0.5 and (got['near_time'] > 0.5).all() and (got['near_time'] < 1.0).all()
    assert _same_bytes(_run(ctx, X, 1, 0.5, look, STEP_E, d_safe=1.0, slots=1), got)


def test_cell_edges_near_miss_pairs(ctx):
    """The step term of the edge: see near_miss_pairs.  A grid of edge d_look + step_max, or a query of the own cell alone, loses
    every one of these pairs."""
    X = near_miss_pairs()
    N = X.shape[2]
    look = LOOK_T
    A, B = X[:, :2, 0::2].transpose(0, 2, 1), X[:, :2, 1::2].transpose(0, 2, 1)        # [row][pair][2]
    assert np.hypot(*(B - A).transpose(2, 0, 1)).min() > look + 5e-3                       # neither row is below d_look
    diff = cells(A[0], EDGE_T) - cells(B[0], EDGE_T)
    assert (np.abs(diff).max(axis=1) == 1).all()                                           # different, neighbouring cells at row 0
    assert {tuple(v) for v in np.abs(diff)} == {(1, 0), (0, 1), (1, 1)}
    narrow = (look + STEP_E) * (1.0 + FL.EDGE_MARGIN)
    assert (np.abs(cells(A[0], narrow) - cells(B[0], narrow)).max(axis=1) >= 2).all()      # half the step term: not neighbours
    got = _run(ctx, X, 1, 0.5, look, STEP_E, d_safe=look)
    ref = _compare(got, X, 1, 0.5, look, STEP_E, 'near miss', d_safe=look)
    assert np.array_equal(got['near_partner'], np.arange(N) ^ 1) and (got['near_count'] == 0).all()
    assert np.abs(got['near_dist'] - 0.99).max() <= 1e-4 and np.abs(got['near_time'] - 0.97 * 0.5).max() <= 1e-4
    assert np.abs(got['near_time'] - ref['near_time']).max() <= 1e-9 * 0.5
    assert _same_bytes(_run(ctx, X, 1, 0.5, look, STEP_E, d_safe=look, slots=1), got)


def test_threshold(ctx):
    """Pairs 2e-6 m inside d_look are seen, pairs 2e-6 m outside are nothing seen."""
    look = 10.0
    X = np.zeros((2, 5, 8))
    for k, (off, ang) in enumerate(((-2e-6, 0.3), (2e-6, 0.3), (-2e-6, 2.0), (2e-6, -1.1))):
        X[:, 0, 2 * k], X[:, 1, 2 * k] = 300.0 * k - 450.0, 7.0 * k
        X[:, 0, 2 * k + 1], X[:, 1, 2 * k + 1] = X[0, 0, 2 * k] + (look + off) * np.cos(ang), X[0, 1, 2 * k] + (look + off) * np.sin(ang)
    got = _run(ctx, X, 1, 1.0, look, 1.0, d_safe=look)
    _compare(got, X, 1, 1.0, look, 1.0, 'threshold', d_safe=look)
    assert list(got['near_partner']) == [1, 0, -1, -1, 5, 4, -1, -1] and list(got['near_count']) == [2, 2, 0, 0, 2, 2, 0, 0]
    assert np.isinf(got['near_dist'][[2, 3, 6, 7]]).all() and np.isnan(got['near_time'][[2, 3, 6, 7]]).all()


def test_ties(ctx):
    X = np.zeros((3, 5, 3))
    X[:, 0, 0] = [-1.0, 0.5, 2.0]                    # the closest approach to both others inside the segment 0 -> 1, at the same s
    X[:, 1, 1], X[:, 1, 2] = 2.0, -2.0
    for slots in (0, 1):
        got = _run(ctx, X, 1, 1.0, 5.0, 2.0, slots=slots)
        assert got['near_partner'][0] == 1 and got['near_dist'][0] == 2.0 and abs(got['near_time'][0] - 2.0 / 3.0) <= 1e-15
    Y = np.zeros((5, 5, 2))
    Y[:, 0, 1] = [3.0, 1.0, 3.0, 1.0, 3.0]           # the same minimum at two rows: the earlier
    for tile in (0, 1, 2):
        got = _run(ctx, Y, 1, 0.5, 5.0, 2.5, tile_rows=tile)
        assert (got['near_dist'] == 1.0).all() and (got['near_time'] == 0.5).all() and list(got['near_partner']) == [1, 0]


@pytest.mark.parametrize('N,n_rows', [(5, 33), (37, 12), (64, 33)])
def test_bit_identity_with_the_in_formation_audit(ctx, N, n_rows):
    """Every aircraft its own formation and a look radius beyond everything: the in-formation audit of one formation of N, bit for bit."""
    X = FA.synthetic_history(1, N, n_rows, seed=N, span=60.0)
    Xd = ctx.dev(X)
    inside = _np(ctx.flight_audit(Xd, N, 0.5, outputs=('sep',)))
    for slots in (0, 4):
        fleet = _np(ctx.fleet_audit(Xd, 1, 0.5, 1e4, STEP, slots=slots))
        ctx.sync()
        assert fleet['near_dist'].tobytes() == inside['sep_dist'].tobytes() and fleet['near_time'].tobytes() == inside['sep_time'].tobytes()
        assert np.array_equal(fleet['near_partner'], inside['sep_partner']) and (fleet['status'] == 0).all()


def test_worlds(ctx):
    """Monte-Carlo replicas that lie on top of each other: one world each, nobody is seen; one world, everybody is 0 m away."""
    one = FA.synthetic_history(1, 3, 9, seed=4, span=300.0)
    X = np.concatenate([one] * 4, axis=2)
    got = _run(ctx, X, 3, 0.5, 20.0, STEP, world=np.arange(4), d_safe=5.0)
    _compare(got, X, 3, 0.5, 20.0, STEP, 'worlds', world=np.arange(4), d_safe=5.0)
    assert (got['near_partner'] == -1).all() and np.isinf(got['near_dist']).all() and (got['near_count'] == 0).all()
    got = _run(ctx, X, 3, 0.5, 20.0, STEP, d_safe=5.0)
    assert (got['near_dist'] == 0.0).all() and (got['near_time'] == 0.0).all() and (got['near_count'] == 9).all()
    assert np.array_equal(got['near_partner'], np.where(np.arange(12) < 3, np.arange(12) + 3, np.arange(12) % 3))     # the smallest index
    got = _run(ctx, X, 3, 0.5, 20.0, STEP, world=np.array([5, -2, 5, -2]))
    assert np.array_equal(got['near_partner'], (np.arange(12) + 6) % 12)


def test_refusals(ctx):
    import d2dhip
    n_form, n_ac, n_rows, dt, look = 6, 2, 9, 0.5, 30.0
    X = FA.synthetic_history(n_form, n_ac, n_rows, seed=8, span=20.0)
    row0 = np.array([0, 1, 0, 2, 0, 1])
    base = dict(row0=row0, g_rows=n_rows + 2, d_safe=10.0)

    def check(Xb, f, bit, **over):
        kw = dict(base, **over)
        got = _run(ctx, Xb, n_ac, dt, look, STEP, **kw)
        sl = slice(f * n_ac, (f + 1) * n_ac)
        assert got['status'][f] == bit and (np.delete(got['status'], f) == 0).all()
        assert np.isnan(got['near_dist'][sl]).all() and np.isnan(got['near_time'][sl]).all()
        assert (got['near_partner'][sl] == -1).all() and (got['near_count'][sl] == -1).all()
        _compare(got, Xb, n_ac, dt, look, STEP, 'refused %d' % bit, **kw)
        # the others: the statement of the history without that formation
        keep = np.delete(np.arange(n_form * n_ac), np.arange(n_form * n_ac)[sl])
        rest = FL.audit(Xb[:, :, keep], n_ac, dt, look, STEP, **dict(kw, row0=np.delete(kw['row0'], f),
                                                                      **({'rows': np.delete(kw['rows'], f)} if 'rows' in kw else {})))
        assert np.isfinite(rest['near_dist']).all()
        assert np.abs(got['near_dist'][keep] - rest['near_dist']).max() <= TOL and np.array_equal(got['near_count'][keep], rest['near_count'])
        assert np.array_equal(got['near_partner'][keep], keep[rest['near_partner']])

    Xb = X.copy(); Xb[7, 1, 1 * n_ac + 1] = np.nan
    check(Xb, 1, d2dhip.FLEET_NONFINITE)
    Xb = X.copy(); Xb[5:, 0, 2 * n_ac] += 2.0                         # one step of up to 5 m along x: longer than step_max ...
    Xb[5:, 1, 2 * n_ac] += 4.0                                        # ... for certain
    assert np.hypot(*(Xb[5, :2, 2 * n_ac] - Xb[4, :2, 2 * n_ac])) > STEP + 0.1
    check(Xb, 2, d2dhip.FLEET_STEP)
    bad0 = row0.copy(); bad0[3] = -1
    check(X, 3, d2dhip.FLEET_BAD_ROW0, row0=bad0)
    bad0 = row0.copy(); bad0[3] = 3                                   # 3 + 9 rows > g_rows = 11
    check(X, 3, d2dhip.FLEET_BAD_ROW0, row0=bad0)
    Xb = X.copy(); Xb[:, 1, 4 * n_ac:5 * n_ac] -= 1e13                # |y / edge| > 2^30
    check(Xb, 4, d2dhip.FLEET_RANGE)
    Xb = X.copy(); Xb[3, 0, 5 * n_ac] = np.inf
    got = _run(ctx, Xb, n_ac, dt, look, STEP, **base)
    assert got['status'][5] & d2dhip.FLEET_NONFINITE and got['status'][5] & d2dhip.FLEET_RANGE and (got['status'][:5] == 0).all()
    # a NaN behind rows[f] is not a refusal
    Xb = X.copy(); Xb[6:, :, 1 * n_ac:2 * n_ac] = np.nan
    rows = np.array([9, 6, 9, 9, 9, 9])
    got = _run(ctx, Xb, n_ac, dt, look, STEP, rows=rows, **base)
    assert (got['status'] == 0).all()
    _compare(got, Xb, n_ac, dt, look, STEP, 'behind', rows=rows, **base)


def test_einval_before_any_launch(ctx):
    import d2dhip
    import torch
    lib = ctx.lib
    n_rows = 4
    X = ctx.zeros(n_rows, 5, 6)
    work = ctx.zeros(1 << 16)
    outs = {k: torch.full((64,), 7, dtype=torch.float64 if k in ('near_dist', 'near_time') else torch.int32, device=ctx.device)
            for k in d2dhip.FLEET_OUT}
    o = d2dhip.FleetOut(**{k: v.data_ptr() for k, v in outs.items()})
    ptr = d2dhip._ptr

    def call(p=None, X_=X, w_=work, o_=o, ctx_=ctx.h, nullp=False):
        p = p or {}
        pp = d2dhip.FleetParams(p.get('n_form', 2), p.get('n_ac', 3), p.get('n_rows', n_rows), p.get('g_rows', n_rows), p.get('tile_rows', 0),
                                p.get('slots', 0), p.get('dt_row', 0.5), p.get('d_look', 10.0), p.get('step_max', 1.0), p.get('d_safe', 0.0))
        assert nullp or (lib.d2d_fleet_audit_workspace(C.byref(pp)) < 0) == bool(p)
        return lib.d2d_fleet_audit(ctx_, None if nullp else C.byref(pp), ptr(X_), None, None, None, ptr(w_), None if o_ is None else C.byref(o_))

    assert call() == 0
    ctx.sync()
    assert bool((outs['status'][:2] == 0).all()) and bool((outs['near_count'][:6] == 0).all())
    for v in outs.values():
        v.fill_(7)
    nan, inf = float('nan'), float('inf')
    bad = [dict(ctx_=None), dict(nullp=True), dict(X_=None), dict(o_=None), dict(w_=None), dict(p=dict(n_form=0)), dict(p=dict(n_ac=0)),
           dict(p=dict(n_ac=65)), dict(p=dict(n_rows=0)), dict(p=dict(g_rows=0))]
    bad += [dict(p={k: v}) for k in ('dt_row', 'd_look', 'step_max') for v in (0.0, -1.0, nan, inf)]
    bad += [dict(p=dict(d_safe=10.5)), dict(p=dict(d_safe=nan)), dict(p=dict(tile_rows=-1)), dict(p=dict(slots=-1))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.d2d_last_error()
    ctx.sync()
    assert all(bool((v == 7).all()) for v in outs.values())          # nothing was launched
    assert lib.d2d_fleet_audit_workspace(None) < 0
    with pytest.raises(d2dhip.D2DError):
        ctx.fleet_audit(X, 3, 0.5, 10.0, 1.0, d_safe=11.0)


def test_workspace_does_not_grow_with_the_rows(ctx):
    import d2dhip
    size = lambda **p: ctx.lib.d2d_fleet_audit_workspace(C.byref(d2dhip.FleetParams(  # noqa: E731
        p.get('n_form', 100), 4, p.get('n_rows', 64), p.get('g_rows', 64), p.get('tile_rows', 8), p.get('slots', 256), 0.5, 10.0, 1.0, 0.0)))
    assert size() == size(n_rows=4096, g_rows=8000) > 0
    assert size(tile_rows=16) > size() and size(slots=1024) > size() and size(n_form=200) > size()


def flown_case(c, X0):
    """Centres (3, 4, 2) and initial states (3, 4, 5): formation 1 is formation 0 moved by (31, 13) m, turned and slower, so that the
    distance between the two changes from row to row; formation 2 is 5 km away."""
    shift = np.array([[0.0, 0.0], [31.0, 13.0], [5000.0, 300.0]])
    cs = c[None] + shift[:, None, :]
    X0s = np.tile(X0, (3, 1, 1)); X0s[:, :, :2] += shift[:, None, :]
    X0s[1, :, 0] += [3.0, -2.0, 1.5, -4.0]; X0s[1, :, 2] += [0.9, -0.6, 1.4, 0.3]; X0s[1, :, 4] = [13.0, 11.0, 14.0, 12.0]
    return cs, X0s


def test_a_flown_history(ctx):
    """Three formations of four through CircularFormationGVF_batch(audit=dict(fleet=...)): the first two fly circles 30 m apart that
    intersect, the third flies 5 km away.  The conflict is reported for the first two, nothing for the third, as the statement has it
    on the downloaded history, and no partner is of the aircraft's own formation."""
    import full_sim as fs
    c = np.array([[0, -20], [25, -40], [25, -80], [0, -100.0]])
    X0 = np.tile([20, 30, -np.pi / 2, 0, 10.0], (4, 1))
    X0[:, 0] += [0.0, 9.0, 21.0, 36.0]; X0[:, 1] += [0.0, -7.0, 5.0, -12.0]
    cs, X0s = flown_case(c, X0)
    look, step_max, d_safe = 40.0, 1.0, 20.0
    out = fs.CircularFormationGVF_batch(cs, 60.0, 15.0, 4, t_start=2.0, t_step=0.05, t_end=2.0 + 40.5 * 0.05, X0=X0s,
                                        audit=dict(d_safe=12.0, fleet=dict(d_look=look, step_max=step_max, d_safe=d_safe)))
    ctx.sync()
    X = out['X'].cpu().numpy()
    assert X.shape == (41, 5, 12)
    rows = np.minimum(out['stop_row'].cpu().numpy(), 41)
    got = _np(out['audit']['fleet'])
    assert set(got) == set(KEYS) and (got['status'] == 0).all()
    assert set(out['audit']) >= {'sep_dist', 'status', 'fleet'}
    Xn = X.copy()
    for f in range(3):
        Xn[rows[f]:, :, 4 * f:4 * f + 4] = np.nan
    _compare(got, Xn, 4, 0.05, look, step_max, 'flown', rows=rows, d_safe=d_safe)
    assert np.isfinite(got['near_dist'][:8]).all() and (got['near_dist'][:8] < look).all() and (got['near_count'][:8] >= 0).all()
    assert (got['near_partner'][:4] // 4 == 1).all() and (got['near_partner'][4:8] // 4 == 0).all()      # never the own formation
    assert (got['near_partner'][8:] == -1).all() and np.isinf(got['near_dist'][8:]).all() and np.isnan(got['near_time'][8:]).all()
    assert (got['near_time'][:8] >= 0.0).all() and (got['near_time'][:8] <= 40 * 0.05 + 1e-12).all()         # from the first row
    plain = fs.CircularFormationGVF_batch(cs, 60.0, 15.0, 4, t_start=2.0, t_step=0.05, t_end=2.0 + 40.5 * 0.05, X0=X0s, audit=dict(d_safe=12.0))
    ctx.sync()
    assert 'fleet' not in plain['audit'] and plain['X'].cpu().numpy().tobytes() == X.tobytes()
    for k in ('sep_dist', 'sep_time', 'sep_partner', 'sep_count'):
        assert plain['audit'][k].cpu().numpy().tobytes() == out['audit'][k].cpu().numpy().tobytes()



def test_the_hook_with_a_plan_and_start_times(ctx):
    """full_sim._fleet_audit as the chain calls it: a plan [N][5][K] (layout='plan') and the formations' own start times on the
    device, which become row0; a start off the row grid is refused by name."""
    import torch
    import full_sim as fs
    n_form, n_ac, K, dt = 5, 3, 12, 0.25
    X = FA.synthetic_history(n_form, n_ac, K, seed=77, span=18.0)
    row0 = np.array([2, 0, 5, 1, 0])
    W = ctx.dev(np.ascontiguousarray(X.transpose(2, 1, 0)))
    t0 = ctx.dev(7.5 + row0 * dt)
    audit = dict(d_safe=3.0, fleet=dict(d_look=25.0, step_max=STEP, d_safe=12.0, world=[0, 0, 0, 1, 0]))
    got = _np(fs._fleet_audit(ctx, audit, W, n_ac, dt, n_form, t_start=t0, layout='plan'))
    ctx.sync()
    ref = _compare(got, X, n_ac, dt, 25.0, STEP, 'plan hook', row0=row0, world=np.array([0, 0, 0, 1, 0]), d_safe=12.0)
    assert np.isfinite(ref['near_dist']).sum() >= 6 and (ref['near_partner'][9:12] == -1).all()
    with pytest.raises(ValueError, match='formation 3 '):
        fs._fleet_audit(ctx, audit, W, n_ac, dt, n_form, t_start=t0 + torch.tensor([0, 0, 0, 0.1, 0], dtype=torch.float64, device=t0.device), layout='plan')


def test_the_tracking_hook(ctx, gold):
    """implement_controller_batch(audit=dict(n_ac=1, fleet=...)): two drones, each its own formation, on references that close."""
    import full_sim as fs
    g = gold('tracking_trace_carestandin')
    T = 50
    time, xr, yr = g['time'][:T], g['x_ref'][:T, :2].copy(), g['y_ref'][:T, :2].copy()
    d0 = np.array([xr[0, 0] - xr[0, 1], yr[0, 0] - yr[0, 1]])
    xr[:, 1] += 0.3 * np.arange(T) * d0[0] / np.hypot(*d0) * 0.1      # the second reference drifts towards the first
    yr[:, 1] += 0.3 * np.arange(T) * d0[1] / np.hypot(*d0) * 0.1
    out = fs.implement_controller_batch(time, xr, yr, (0.5, -0.3), g['X'][0][:2], audit=dict(n_ac=1, fleet=dict(d_look=100.0, step_max=3.0)))
    ctx.sync()
    X = out['X'].cpu().numpy()
    got = _np(out['audit']['fleet'])
    _compare(got, X, 1, float(time[1] - time[0]), 100.0, 3.0, 'tracking hook')
    assert list(got['near_partner']) == [1, 0] and (got['near_dist'] < 25.0).all() and 'err_max' in out['audit']


@pytest.mark.parametrize('t_step', [0.1, 0.05])
def test_the_chain_places_formations_by_their_own_start(ctx, t_step):
    """full_sim_phases_batch(audit=dict(fleet=...)) WITHOUT a field or moving discs: every formation's transition still starts where
    its own phase 1 ended, so the plan and phase 2 are compared at row0 = (t2 - min t2) / dt2 -- or, when a formation is off that
    grid, the call refuses it by name.  Which of the two happens follows from the stop rows, which the test reads from phase 1."""
    import d2d.opty_utils as d2ou
    import full_sim as fs
    import multi_opt_planner as mop
    import nlp_groups_wind_ref as G
    n_ac, c, X1_f, X2_f, X0B, _ = G.mission_inputs()
    cB = np.stack([c, c, c])
    r, v, t_opt = 60, 15, 6
    ph1 = fs.CircularFormationGVF_batch(cB, r, v, n_ac, X0f=np.broadcast_to(X1_f[None, :, :3], (3, n_ac, 3)), X0=X0B, record=(), t_step=t_step)
    ctx.sync()
    t2 = (np.minimum(ph1['stop_row'].cpu().numpy(), len(ph1['time'])) - 1) * t_step
    mop.trap_4.t1 = t_opt
    _, dt2, _ = d2ou.planner_timing(mop.trap_4.t0, t_opt, mop.trap_4.hz)
    u = (t2 - t2.min()) / dt2
    off = np.nonzero(np.abs(u - np.rint(u)) > 1e-9)[0]
    look, step_max = 60.0, 3.0
    run = lambda: fs.full_sim_phases_batch(cB, r, v, n_ac, X1_f, mop.trap_4, X2_f, t_opt, X0=X0B, t_step=t_step,      # noqa: E731
                                           audit=dict(fleet=dict(d_look=look, step_max=step_max)))
    print('t2', t2, 'rows', u)
    if off.size:
        with pytest.raises(ValueError, match='formation %d ' % off[0]):
            run()
        return
    out = run()
    ctx.sync()
    row0 = np.rint(u).astype(int)
    Xs = out['plan']['Xs'].cpu().numpy()
    for name, X in (('plan', np.ascontiguousarray(Xs.transpose(2, 1, 0))), ('phase2', out['phase2']['X'].cpu().numpy())):
        got = _np(out['audit'][name]['fleet'])
        assert (got['status'] == 0).all(), (name, got['status'])
        _compare(got, X, n_ac, float(dt2), look, step_max, 'chain ' + name, row0=row0)
        seen = got['near_partner'] >= 0
        assert (got['near_partner'][seen] // n_ac != np.arange(12)[seen] // n_ac).all()      # never the own formation
        print(name, 'row0', row0, 'seen', int(seen.sum()), 'closest', got['near_dist'].min())
