"""The CPU statement of the Dubins start (tests/nlp_guess_ref.py) on the committed parity cases (tests/nlp_guess_cases.py): what the
table claims, the geometry of every guess, the refusals, the determinacy the GPU comparison rests on, and the point of it -- fewer
Newton steps of oracle.nlp.solve to the same minimum."""
import os
import re

import numpy as np
import pytest

import nlp_guess_cases as GC
import nlp_guess_ref as GR
from oracle import nlp as ON

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(ci, v) for ci in range(len(GC.CASES)) for v in GC.VARIANTS]


def test_constants_match_the_header_and_the_binding():
    import d2dhip
    for name in ('SC_X0', 'SC_X1', 'SC_VREF', 'SC_VSP', 'SC_KV', 'SC_WX', 'SC_WY', 'SC_PHIMAX', 'SC_VMIN', 'SC_VMAX'):
        assert getattr(GR, name) == getattr(d2dhip, name), name
    assert GC.STRIDE == d2dhip.SCEN_STRIDE
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    macro = lambda n: float(re.search(r'#define D2D_GUESS_%s (\S+)' % n, hdr).group(1))     # noqa: E731
    for i, name in enumerate(GR.STATUS):
        assert macro(name) == i == getattr(d2dhip, 'GUESS_' + name)
    assert d2dhip.GUESS_STATUS == GR.STATUS and d2dhip.GUESS_WORDS == GR.WORDS
    assert (macro('KAPPA'), macro('TURN_TOL'), macro('ROUNDS'), macro('GROW'), macro('GROW_MAX')) == (GR.KAPPA, GR.TURN_TOL, GR.ROUNDS, GR.GROW, GR.GROW_MAX)
    assert d2dhip.GUESS_KAPPA == GR.KAPPA and GR.G_ACC == ON.G_ACC


def test_the_table_every_word_and_every_status():
    got = {v: [] for v in GC.VARIANTS}
    for ci, variant in ALL:
        case = GC.CASES[ci]
        _, o = GC.one(case, variant, 121)
        want = case[7 if variant == 'plain' else 8]
        assert (o['status'], o['word']) == want, (ci, variant, o)
        got[variant].append(want)
    assert {w for _, w in got['plain']} >= set(range(6)), 'each of the six words is the chosen one at least once'
    for variant in GC.VARIANTS:
        assert {s for s, _ in got[variant]} >= {GR.FIT, GR.SHORT, GR.LOOSE, GR.LOOSE_UNMET, GR.LINE}, variant
    assert sum(1 for c in GC.CASES if c[2] != (0.0, 0.0)) >= 8        # wind among them


@pytest.mark.parametrize('N', GC.NS)
def test_determinacy(N):
    """No search evaluation within F_MIN v T of zero, and the second-best admissible word MARGIN_MIN longer at the bracket ends and
    at the result: what makes status, word and every decision of the search the same on any machine.  No case is exempt."""
    for ci, variant in ALL:
        f, m = GC.determined(GC.CASES[ci], variant, N)
        assert f >= GC.F_MIN and m >= GC.MARGIN_MIN, (ci, variant, N, f, m)


@pytest.mark.parametrize('N', GC.NS)
def test_geometry_of_every_guess(N):
    """Ends, net turning, length and collocation residual of every case.

    Spacing ds = L / (N - 1) along a path of curvature at most 1 / rho, so the heading changes by at most dpsi = ds / rho between two
    nodes: with the pinned ends equal to the poses that is the net turning psi1 - psi0 without a wrap.  A chord of an arc of angle
    theta is 2 rho sin(theta / 2) >= rho theta (1 - theta^2 / 24): the air-frame polyline is shorter than L by at most
    L ds^2 / (24 rho^2), and longer by nothing.  Residuals in the oracle's form (divided by h).  Position: the displacement of a step
    is w h + chord e, with e a unit vector within dpsi of the node's heading u (the chord of a path whose heading stays within dpsi of
    u), so c_xy = chord e / h - v u and |c_xy| <= |chord / h - v| + v |e - u| <= |ds / h - v| + ds dpsi^2 / (24 h) + v dpsi: the
    node spacing's heading change times v, plus what the spacing misses v h by (nothing for FIT, (L - v T) / T for SHORT).
    Heading: |(psi_i - psi_{i-1}) / h| <= dpsi / h and |g tan(phi_i) / v| = v / rho on an arc, 0 on the straight, so |c_psi| <=
    dpsi / h + v / rho (the two cancel inside an arc; the bound is what a step across a junction can reach)."""
    h = GC.step(N)
    met = {GR.FIT: 0, GR.LOOSE: 0}
    for ci, variant in ALL:
        case = GC.CASES[ci]
        W, o = GC.one(case, variant, N)
        r = GC.row(case)
        assert np.array_equal(W[:3, 0], r[GR.SC_X0:GR.SC_X0 + 3]) and np.array_equal(W[:3, -1], r[GR.SC_X1:GR.SC_X1 + 3]), (ci, variant)
        assert np.all(W[4] == o['v']) and GC.V_BOX[0] <= o['v'] <= GC.V_BOX[1]
        t = np.arange(N) * h
        air = np.stack([W[0] - r[GR.SC_WX] * t, W[1] - r[GR.SC_WY] * t])
        chords = np.sqrt((np.diff(air, axis=1) ** 2).sum(0))
        pb = ON.problem_from_row(r, N, h)
        c = np.abs(ON.constraints(pb, W.T))
        if o['status'] == GR.LINE:
            ground = np.sqrt((np.diff(W[:2], axis=1) ** 2).sum(0)).sum()
            assert abs(ground - o['L']) <= 1e-9 * max(o['L'], 1.0) and np.all(W[3] == 0.0) and o['word'] == -1 and np.isinf(o['rho'])
            continue
        phi_lim = min(abs(case[5][0]), abs(case[5][1])) if variant == 'opts' else GC.PHIMAX
        assert np.abs(W[3]).max() <= GR.KAPPA * phi_lim + 1e-12          # at most the fraction kappa of the limit
        ds = o['L'] / (N - 1)
        dpsi = ds / o['rho']
        assert np.abs(np.diff(W[2])).max() <= dpsi + 1e-9, (ci, variant)
        short = o['L'] * ds ** 2 / (24.0 * o['rho'] ** 2)
        assert o['L'] - short - 1e-9 <= chords.sum() <= o['L'] + 1e-9, (ci, variant, chords.sum(), o['L'], short)
        if dpsi <= 1.0:                # every chord, the last one too: the path built in the air frame meets p1 - w T
            assert np.all(chords <= ds + 1e-9) and np.all(chords >= ds * (1.0 - dpsi ** 2 / 24.0) - 1e-9), (ci, variant)
        slack = abs(ds / h - o['v']) + ds * dpsi ** 2 / (24.0 * h)
        assert c[:, :2].max() <= slack + o['v'] * dpsi + 1e-9, (ci, variant, c[:, :2].max(), slack + o['v'] * dpsi)
        assert c[:, 2].max() <= dpsi / h + o['v'] / o['rho'] + 1e-9, (ci, variant)
        if o['status'] in (GR.FIT, GR.LOOSE):     # the side where the path is no longer than v T; L = v T to the last bracket's width
            assert o['L'] <= o['v'] * GC.T0 * (1.0 + 1e-14), (ci, variant, o)     # unless L* jumps inside it (case 1 with its bounds)
            met[o['status']] += abs(o['L'] - o['v'] * GC.T0) <= 1e-3
        if o['status'] == GR.SHORT:
            assert o['v'] == GC.V_BOX[1] and o['L'] > o['v'] * GC.T0
        if o['status'] == GR.LOOSE_UNMET:
            assert o['L'] < o['v'] * GC.T0
    assert met[GR.FIT] >= 8 and met[GR.LOOSE] >= 8, met


def test_refusals_leave_W_untouched():
    rows = np.concatenate([GC.refused_rows(), GC.row(GC.CASES[1])[None]])
    B, N = rows.shape[0], 17
    W = np.full((B, 5, N), -7.25)
    W, out = GR.guess(rows, N, GC.step(N), W=W)
    assert np.all(out['status'][:-1] == GR.INVALID) and out['status'][-1] == GC.CASES[1][7][0]
    assert np.all(W[:-1] == -7.25) and not np.any(W[-1] == -7.25)
    assert np.all(out['word'][:-1] == -1) and all(np.all(np.isnan(out[k][:-1])) for k in ('v', 'rho', 'L', 't_nat'))
    for Nb, hb in ((1, 0.1), (17, 0.0), (17, -0.1), (17, np.nan)):           # the call's own N and h: every row
        Wb, ob = GR.guess(rows[-1:], Nb, hb, W=np.full((1, 5, Nb), -7.25))
        assert ob['status'][0] == GR.INVALID and np.all(Wb == -7.25)
    bnd = np.tile([0.0, 0.5, 0.0, 0.0], (1, 1))                             # an interval that holds no bank to either side
    assert GR.guess(rows[-1:], N, GC.step(N), bounds=bnd)[1]['status'][0] == GR.INVALID
    with pytest.raises(ValueError):
        GR.guess(rows[-1:], N, GC.step(N), kappa=1.5)


def test_preferred_speed_rule():
    r = GC.row(GC.CASES[7])              # KV = 1: VSP
    N, h = 33, GC.step(33)
    assert GR.guess_one(r, N, h)[1]['t_nat'] == GR.guess_one(r, N, h, v_pref=GC.VSP)[1]['t_nat']
    r[GR.SC_KV], r[GR.SC_VREF] = 0.0, 10.5
    assert GR.guess_one(r, N, h)[1]['t_nat'] == GR.guess_one(r, N, h, v_pref=10.5)[1]['t_nat']
    r[GR.SC_VREF] = 0.0
    assert GR.guess_one(r, N, h)[1]['t_nat'] == GR.guess_one(r, N, h, v_pref=12.0)[1]['t_nat']        # the middle of [9, 15]
    assert GR.guess_one(r, N, h, v_pref=99.0)[1]['t_nat'] == GR.guess_one(r, N, h, v_pref=15.0)[1]['t_nat']   # clamped


def test_floors_are_small_and_measured():
    f = GR.floors(GC.row(GC.CASES[2]), 65, GC.step(65))
    assert f.shape == (len(GR.QUANTITIES),) and 0.0 < f.max() <= 1e-10, f


def test_oracle_steps_from_both_starts():
    """The first 32 problems of synth.nlp_problems(seed=0), 121 nodes, through oracle.nlp.solve from the host dog-leg and from the
    Dubins start: the same verdicts, the same minima, at most 0.75 of the Newton steps (measured 0.60: 4836 -> 2914; longest 182 -> 111)."""
    from d2dhip import synth
    n, N = 32, 121
    rows, W0, h = synth.nlp_problems(n, N, seed=0)
    Wd, out = GR.guess(rows, N, h)
    assert np.all(out['status'] <= GR.SHORT)
    steps = np.zeros((2, n), int)
    for b in range(n):
        pb = ON.problem_from_row(rows[b], N, h)
        _, tri = ON.solve(pb, W0[b].T.copy())
        _, dub = ON.solve(pb, Wd[b].T.copy())
        assert tri['status'] == dub['status'], (b, tri['status'], dub['status'])
        assert abs(tri['cost'] - dub['cost']) <= 1e-7, (b, tri['cost'], dub['cost'])
        steps[:, b] = tri['inner'], dub['inner']
    print('steps: dog-leg %d, Dubins %d (%.3f); longest %d -> %d' % (steps[0].sum(), steps[1].sum(), steps[1].sum() / steps[0].sum(),
                                                                     steps[0].max(), steps[1].max()))
    assert steps[1].sum() <= 0.75 * steps[0].sum()
    assert steps[1].max() < steps[0].max()
