"""GPU parity of d2d_fleet_tracks (csrc/fleet_tracks.hip) with its CPU statement tests/fleet_tracks_ref.py (brute force over all pairs).

Byte parity.  The device evaluates the audit's segment rule with fused multiply-adds, the statement with numpy's separate operations;
on fleet_tracks_ref.lattice_history every product of that rule is exact, so both give the same bits and EVERY output is compared byte
for byte (NaNs as NaNs), chord_err included -- its sequence is stated without fused operations and followed by the kernel on any
history.  On a history in general position (flight_audit_ref.synthetic_history) the fused and the separate d^2 differ in the last
bits: there the integer outputs, the knots and chord_err are compared byte for byte and part_dist / part_time to the fleet audit's
tolerances (1e-10 m, 1e-9 rows)."""
import ctypes as C

import numpy as np
import pytest

import fleet_audit_ref as FL
import fleet_tracks_ref as FT
import flight_audit_ref as FA

pytestmark = pytest.mark.gpu
KEYS = ('knots', 'disc', 'partner', 'part_dist', 'part_time', 'chord_err', 'n_conf', 'status')
STEP = 3.0          # lattice_history moves 2 m per row and axis: 2 sqrt 2 = 2.83


@pytest.fixture(scope='module')
def ctx():
    import d2dhip
    return d2dhip.default_context()


def _run(ctx, X, n_ac, dt, d_look, step_max, r_disc=2.0, fn='fleet_tracks', **kw):
    import torch
    dev = dict(kw)
    for k in ('rows', 'row0', 'world', 'prio'):
        if dev.get(k) is not None:
            dev[k] = torch.as_tensor(np.ascontiguousarray(dev[k]), dtype=torch.int32).to(ctx.device)
    a = (ctx.dev(np.ascontiguousarray(X)), n_ac, dt, d_look, step_max) + ((r_disc,) if fn == 'fleet_tracks' else ())
    out = getattr(ctx, fn)(*a, **dev)
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ref(X, n_ac, dt, d_look, step_max, r_disc=2.0, **kw):
    return FT.tracks(X, n_ac, dt, d_look, step_max, r_disc, **{k: v for k, v in kw.items() if k not in ('tile_rows', 'slots')})


def _bytes(a):
    return (np.where(np.isnan(a), np.nan, a) if a.dtype.kind == 'f' else a).tobytes()


def _same(a, b, keys=KEYS, what=''):
    for k in keys:
        assert a[k].shape == b[k].shape and _bytes(a[k]) == _bytes(b[k]), (what, k, a[k], b[k])


def lattice_case(n_form, n_ac, n_rows, n_knot):
    """A lattice history dense enough that formations meet within d_look = 9 m, with windows, offsets, worlds and priorities; rows
    behind a formation's window are NaN (a status there: such a row was read)."""
    N = n_form * n_ac
    seed = 1000 * n_form + 10 * n_ac + n_rows
    X = FT.lattice_history(n_form, n_ac, n_rows, seed, span=int(max(6, 3 * np.sqrt(N))))
    rng = np.random.default_rng(seed + 1)
    rows = rng.integers(n_knot, n_rows + 1, n_form)
    row0 = rng.integers(0, n_rows // 2 + 1, n_form)
    if n_form > 3:
        rows[3] = n_knot - 1                                         # one SHORT formation
    world = (np.arange(n_form) // 3) % 2 if n_form > 6 else np.zeros(n_form, int)
    prio = rng.integers(0, max(2, n_form // 2), n_form)              # ties: the formation index decides
    for f in range(n_form):
        X[rows[f]:, :, f * n_ac:(f + 1) * n_ac] = np.nan
    return X, dict(rows=rows, row0=row0, world=world, prio=prio)


@pytest.mark.parametrize('n_mov', [1, 3, 8])
@pytest.mark.parametrize('n_form,n_ac,n_rows', [(2, 1, 4), (7, 1, 9), (12, 3, 12), (2, 64, 4), (48, 1, 24)])
def test_every_output_is_the_statements_byte_for_byte(ctx, n_form, n_ac, n_rows, n_mov):
    n_knot = 4
    X, kw = lattice_case(n_form, n_ac, n_rows, n_knot)
    kw.update(n_mov=n_mov, n_knot=n_knot, kind=n_mov % 2, t0=3.25)
    got = _run(ctx, X, n_ac, 0.5, 9.0, STEP, 2.5, **kw)
    ref = _ref(X, n_ac, 0.5, 9.0, STEP, 2.5, **kw)
    _same(got, ref, what='clocks')
    assert ((got['status'] & ~FT.SHORT) == 0).all()
    if n_form >= 7:
        assert (ref['n_conf'] > 0).any() and (ref['n_conf'] == 0).any()            # not vacuous
    bare = dict(n_mov=n_mov, n_knot=n_rows if n_rows <= 32 else 32, t0=0.0)
    Xb = FT.lattice_history(n_form, n_ac, n_rows, 77 + n_form, span=int(max(6, 3 * np.sqrt(n_form * n_ac))))
    _same(_run(ctx, Xb, n_ac, 0.5, 9.0, STEP, **bare), _ref(Xb, n_ac, 0.5, 9.0, STEP, **bare), what='bare')


def test_a_history_in_general_position(ctx):
    """Positions that are no lattice: what the fused d^2 can move is held to the fleet audit's tolerances, the rest to the byte."""
    n_form, n_ac, n_rows = 10, 3, 12
    X = FA.synthetic_history(n_form, n_ac, n_rows, 4242, span=30.0)
    kw = dict(n_mov=4, n_knot=5, t0=1.7, prio=np.arange(n_form)[::-1] // 2)
    got = _run(ctx, X, n_ac, 0.3, 25.0, 4.3, 3.0, **kw)
    ref = _ref(X, n_ac, 0.3, 25.0, 4.3, 3.0, **kw)
    _same(got, ref, ('partner', 'n_conf', 'status', 'knots', 'disc', 'chord_err'))
    on = ref['partner'] >= 0
    assert on.sum() > 10 and (ref['chord_err'][on] > 0.1).any()
    assert np.abs(got['part_dist'][on] - ref['part_dist'][on]).max() <= 1e-10
    assert np.abs(got['part_time'][on] - ref['part_time'][on]).max() <= 1e-9 * 0.3 * 1e3        # (s* of a slow relative motion: 1e-6 rows)
    assert np.isinf(got['part_dist'][~on]).all() and np.isnan(got['part_time'][~on]).all()


def test_the_grid_only_schedules(ctx):
    n_form, n_ac, n_rows = 11, 3, 14
    X, kw = lattice_case(n_form, n_ac, n_rows, 4)
    kw.update(n_mov=3, n_knot=4)
    g_rows = int((kw['row0'] + kw['rows']).max())
    first = _run(ctx, X, n_ac, 0.5, 9.0, STEP, **kw)
    _same(first, _ref(X, n_ac, 0.5, 9.0, STEP, **kw))
    assert (first['n_conf'] > 1).any()
    for tile in (1, 3, 0, g_rows + 5):
        for slots in (1, 2, 0):
            _same(_run(ctx, X, n_ac, 0.5, 9.0, STEP, tile_rows=tile, slots=slots, **kw), first, what=(tile, slots))
    _same(_run(ctx, X, n_ac, 0.5, 9.0, STEP, **kw), first, what='again')


def _static(points, n_rows=3):
    X = np.zeros((n_rows, 5, len(points)))
    X[:, 0], X[:, 1] = np.asarray(points, dtype=np.float64).T[:, None, :]
    return X


@pytest.mark.parametrize('n_mov', [1, 8])
def test_list_edges(ctx, n_mov):
    """0, exactly n_mov, n_mov + 1 and 3 n_mov partners within d_look of the last (lowest) formation, at distinct distances."""
    for P in (0, n_mov, n_mov + 1, 3 * n_mov):
        X = _static([(1.0 + 0.5 * p, 0.0) for p in range(P)] + [(0.0, 0.0)], 2)
        kw = dict(n_mov=n_mov, n_knot=2)
        got = _run(ctx, X, 1, 1.0, 20.0, 1.0, **kw)
        _same(got, _ref(X, 1, 1.0, 20.0, 1.0, **kw), what=P)
        assert got['n_conf'][P] == min(P, n_mov + 1)
        assert got['partner'][P].tolist() == (list(range(P)) + [-1] * n_mov)[:n_mov]
        for tile in (1, 2):
            _same(_run(ctx, X, 1, 1.0, 20.0, 1.0, tile_rows=tile, slots=1, **kw), got, what=(P, tile))


def test_one_partner_seen_by_two_aircraft_in_two_tiles(ctx):
    """Aircraft 2 of formation 1 is 3 m from aircraft 0 at row 0; aircraft 3 is 2 m from it at row 5.  One entry, the smaller key."""
    X = np.zeros((6, 5, 4))
    X[:, 0, 1] = 100.0                               # aircraft 1 is far away
    X[:, 1, 2] = [3, 5, 7, 9, 11, 13]                # aircraft 2 leaves
    X[:, 1, 3] = [-12, -10, -8, -6, -4, -2]          # aircraft 3 arrives
    for tile in (0, 2, 1):
        got = _run(ctx, X, 2, 1.0, 3.5, 2.5, n_mov=2, n_knot=2, tile_rows=tile)
        assert got['partner'].tolist() == [[-1, -1], [0, -1]] and got['n_conf'].tolist() == [0, 1]
        assert got['part_dist'][1, 0] == 2.0 and got['part_time'][1, 0] == 5.0
    _same(got, _ref(X, 2, 1.0, 3.5, 2.5, n_mov=2, n_knot=2))


def test_exact_ties_the_look_radius_and_an_interior_approach(ctx):
    # mirror geometry on whole metres: d^2 = 9 three times; the order is by time, then by index
    X = np.zeros((3, 5, 4))
    X[:, 0, 0], X[:, 1, 1], X[:, 0, 2] = [5, 4, 3], [4, 3, 3], [-4, -3, -3]
    got = _run(ctx, X, 1, 1.0, 3.5, 1.5, n_mov=3, n_knot=2)
    assert got['partner'][3].tolist() == [1, 2, 0] and got['part_time'][3].tolist() == [1.0, 1.0, 2.0] and got['part_dist'][3].tolist() == [3.0] * 3
    _same(got, _ref(X, 1, 1.0, 3.5, 1.5, n_mov=3, n_knot=2))
    # a pair exactly at d_look (3-4-5): strict, not listed; one ulp more: listed
    X = _static([(0.0, 0.0), (3.0, 4.0)])
    assert _run(ctx, X, 1, 1.0, 5.0, 1.0, n_mov=1, n_knot=2)['partner'].tolist() == [[-1], [-1]]
    got = _run(ctx, X, 1, 1.0, np.nextafter(5.0, 6.0), 1.0, n_mov=1, n_knot=2)
    assert got['partner'].tolist() == [[-1], [0]] and got['part_dist'][1, 0] == 5.0
    # crossing legs that tunnel between rows 1 and 2: no row is below d_look = 1 m (the nearest is exactly 1 m), the interior approach is
    X = np.zeros((5, 5, 2))
    X[:, 0, 0], X[:, 1, 1] = 2 * np.arange(5) - 4, 2 * np.arange(5) - 3
    got = _run(ctx, X, 1, 0.5, 1.0, 3.0, n_mov=1, n_knot=3, t0=10.0)
    assert got['partner'].tolist() == [[-1], [0]] and got['part_dist'][1, 0] == np.sqrt(0.5) and got['part_time'][1, 0] == 1.75 * 0.5
    _same(got, _ref(X, 1, 0.5, 1.0, 3.0, n_mov=1, n_knot=3, t0=10.0))


def test_priority_and_worlds(ctx):
    # formation 1 at the origin; formation 2, 1 m away, ranks below it; formation 0, 3 m away, above: only formation 0 is listed
    X = _static([(3.0, 0.0), (0.0, 0.0), (0.0, 1.0)])
    got = _run(ctx, X, 1, 1.0, 5.0, 1.0, n_mov=2, n_knot=2)
    assert got['partner'].tolist() == [[-1, -1], [0, -1], [1, 0]]
    _same(got, _ref(X, 1, 1.0, 5.0, 1.0, n_mov=2, n_knot=2))
    # equal prio falls back to the formation index
    X = _static([(0.0, 0.0), (2.0, 0.0), (4.0, 0.0)])
    got = _run(ctx, X, 1, 1.0, 5.0, 1.0, n_mov=2, n_knot=2, prio=[7, 7, 1])
    assert got['partner'].tolist() == [[2, -1], [0, 2], [-1, -1]]
    _same(got, _ref(X, 1, 1.0, 5.0, 1.0, n_mov=2, n_knot=2, prio=[7, 7, 1]))
    # worlds do not see each other
    got = _run(ctx, X, 1, 1.0, 5.0, 1.0, n_mov=2, n_knot=2, world=[0, 1, 0])
    assert got['partner'].tolist() == [[-1, -1], [-1, -1], [0, -1]]


def test_refusals_and_windows(ctx):
    # a refused formation: NaN / -1, absent discs, and the others do not see it
    X = _static([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)], 4)
    X[2, 0, 1] = np.nan
    got = _run(ctx, X, 1, 1.0, 5.0, 1.0, n_mov=2, n_knot=3, t0=1.0)
    assert got['status'].tolist() == [0, FL.NONFINITE, 0] and got['n_conf'].tolist() == [0, -1, 1]
    assert got['partner'].tolist() == [[-1, -1], [-1, -1], [0, -1]] and np.isnan(got['part_dist'][1]).all() and np.isnan(got['chord_err'][1]).all()
    assert (got['disc'][1, :, 0] == 0).all() and got['knots'][1, 0, :, 0].tolist() == [1.0, 2.0, 3.0]
    _same(got, _ref(X, 1, 1.0, 5.0, 1.0, n_mov=2, n_knot=3, t0=1.0))
    # fewer valid rows than knots: SHORT, its own outputs refused, but the formation it outranks still sees it
    kw = dict(rows=[2, 4, 4], n_mov=2, n_knot=3)
    X = _static([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)], 4)
    got = _run(ctx, X, 1, 1.0, 5.0, 1.0, **kw)
    assert got['status'].tolist() == [FT.SHORT, 0, 0] and got['partner'].tolist() == [[-1, -1], [0, -1], [1, 0]]
    _same(got, _ref(X, 1, 1.0, 5.0, 1.0, **kw))
    # offsets: the partner's window starts after the formation's (held at its first row) and ends before it (held at its last)
    X = np.zeros((7, 5, 2))
    X[:5, 0, 0], X[:5, 1, 0] = [0, 1, 2, 3, 4], [0, 1, 0, 1, 0]
    X[:, 0, 1], X[:, 1, 1] = 2.0, 0.5
    kw = dict(rows=[5, 7], row0=[1, 0], n_mov=1, n_knot=4)
    got = _run(ctx, X, 1, 1.0, 3.0, 1.5, **kw)
    assert got['knots'][1, 0].tolist() == [[0.0, 0.0, 0.0], [2.0, 1.0, 1.0], [4.0, 3.0, 1.0], [6.0, 4.0, 0.0]]       # rows 0, 2, 4, 6: local 0 (held), 1, 3, 4 (held)
    _same(got, _ref(X, 1, 1.0, 3.0, 1.5, **kw))


def test_einval_before_anything_is_launched(ctx):
    import d2dhip
    X = ctx.dev(_static([(0.0, 0.0), (1.0, 0.0)], 4))
    ok = dict(n_mov=2, n_knot=3, kind=1, t0=0.0)
    for bad in (dict(n_mov=0), dict(n_mov=d2dhip.MAX_MOV + 1), dict(n_knot=1), dict(n_knot=d2dhip.MOV_MAX_KNOT + 1), dict(kind=2), dict(kind=-1),
                dict(t0=float('inf')), dict(t0=float('nan')), dict(tile_rows=-1), dict(slots=-1), dict(g_rows=0)):
        with pytest.raises(d2dhip.D2DError):
            ctx.fleet_tracks(X, 1, 1.0, 5.0, 1.0, 2.0, **{**ok, **bad})
    for a in ((1, 1.0, 5.0, 1.0, 0.0), (1, 1.0, 5.0, 1.0, float('nan')), (1, 0.0, 5.0, 1.0, 2.0), (1, 1.0, -1.0, 1.0, 2.0), (1, 1.0, 5.0, float('inf'), 2.0)):
        with pytest.raises(d2dhip.D2DError):
            ctx.fleet_tracks(X, *a, **ok)
    p = d2dhip.FleetParams(2, 65, 4, 4, 0, 0, 1.0, 5.0, 1.0, 0.0)
    assert ctx.lib.d2d_fleet_tracks_workspace(C.byref(p), 2) < 0
    p = d2dhip.FleetParams(2, 1, 4, 4, 0, 0, 1.0, 5.0, 1.0, 0.0)
    w1, w8 = ctx.lib.d2d_fleet_tracks_workspace(C.byref(p), 1), ctx.lib.d2d_fleet_tracks_workspace(C.byref(p), 8)
    assert 0 < w1 < w8 and ctx.lib.d2d_fleet_tracks_workspace(C.byref(p), 9) < 0
    ctx.sync()


def test_consistency_with_the_fleet_audit(ctx):
    """Where every other formation outranks f, entry 0 of f is the nearest approach of any of f's aircraft: fleet_audit's bytes."""
    n_form, n_ac, n_rows = 5, 3, 10
    X = FA.synthetic_history(n_form, n_ac, n_rows, 99, span=14.0)
    aud = _run(ctx, X, n_ac, 0.5, 25.0, 4.3, fn='fleet_audit')
    assert np.isfinite(aud['near_dist']).all()
    for f in range(n_form):
        got = _run(ctx, X, n_ac, 0.5, 25.0, 4.3, n_mov=2, n_knot=4, prio=(np.arange(n_form) == f).astype(int))
        a = f * n_ac + int(np.argmin(aud['near_dist'][f * n_ac:(f + 1) * n_ac]))
        assert got['part_dist'][f, 0].tobytes() == aud['near_dist'][a].tobytes() and got['partner'][f, 0] == aud['near_partner'][a]
        assert got['part_time'][f, 0].tobytes() == aud['near_time'][a].tobytes()


def test_the_tables_are_usable(ctx):
    """mov_sample on the written knots gives the partner's history at the knot rows exactly (one knot per row, dyadic times), and
    nlp_solve_groups_moving refuses no scenario that is handed these tables, absent slots included."""
    import d2dhip
    import nlp_moving_ref as M
    R, n_ac, N, h = 4, 3, 13, 0.5
    rows = []
    for r in range(R):
        for a in range(n_ac):
            th = 0.8 * r + 0.1
            c, s = np.cos(th), np.sin(th)
            off = 4.0 * (a - 1)
            rows.append(M.row(1, p0=(-36 * c - off * s, -36 * s + off * c, th), p1=(36 * c - off * s, 36 * s + off * c, th), N=N))
    rows = np.stack(rows)
    W0 = np.stack([M.straight_guess(r, N).T for r in rows])
    W0[:, :2] = np.round(W0[:, :2] * 4.0) / 4.0                   # quarter metres: the sampler's multiply-add is exact on them
    W = ctx.dev(W0)
    tr = ctx.fleet_tracks(W, n_ac, h, 12.0, 7.5, 5.0, n_mov=4, n_knot=N, t0=2.0, layout='plan')
    ctr = ctx.mov_sample(tr['knots'], tr['disc'], 2.0, N, h).cpu().numpy()
    partner, n_conf = tr['partner'].cpu().numpy(), tr['n_conf'].cpu().numpy()
    assert (tr['status'].cpu().numpy() == 0).all() and n_conf[0] == 0 and (n_conf[1:] > 0).all() and (partner == -1).any()
    for f in range(R):
        for m in range(4):
            e = partner[f, m]
            want = W0[e, :2] if e >= 0 else np.zeros((2, N))
            assert np.array_equal(ctr[f, m], want), (f, m)
    out = ctx.nlp_solve_groups_moving(ctx.dev(rows), W, h, n_ac, tr['knots'], tr['disc'], None, 2.0, max_sweeps=2)
    ctx.sync()
    assert (out['status'].cpu().numpy() != d2dhip.ST_NONFINITE).all() and np.isfinite(out['cost'].cpu().numpy()).all()
