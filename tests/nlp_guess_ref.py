"""CPU statement of d2d_nlp_guess_dubins (csrc/nlp_guess.hip; include/d2d.h states the call): the start of a collocation solve
built from a Dubins path.  numpy only.  The kernel follows this file decision for decision; DESIGN 5.23 has the rule in words.

The model's phi and v are free controls at every node, so a path of circular arcs at (a fraction kappa of) the bank limit and a
straight line, flown at one speed, is almost a feasible point of the NLP.  In a constant wind w and at the fixed duration
T = (N - 1) h a ground path is an air path plus w t: the path is built in the air frame from p0 to p1' = p1 - w T and node i is
shifted by w i h.

Words.  With turn signs a, b in {+1 (L), -1 (R)} the circle centres are c0 = p0 + a rho n(psi0), c1 = p1' + b rho n(psi1),
n(psi) = (-sin psi, cos psi); D = c1 - c0, l = |D|, gamma = atan2(D).  A point of a circle of sign s at heading chi is
c - s rho n(chi), so the straight of a C S C word is  p u(chi) = D + (a - b) rho n(chi):  a = b gives chi = gamma, p = l; a = -b gives
p = sqrt(l^2 - 4 rho^2) (l >= 2 rho) and chi = gamma + a atan2(2 rho, p).  A C C C word (s, -s, s) has its middle centre at 2 rho
from both: with A = acos(l / 4 rho) (l <= 4 rho) and the middle arc the long one, pi + 2 A, the headings at the two junctions are
chi1 = gamma + s A + s pi/2 and chi2 = gamma + pi - s A + s pi/2.  The arcs turn t = mod(a (chi - psi0)), q = mod(b (psi1 - chi))
(chi1 and chi2 in the C C C words), mod into [0, 2 pi).

The NLP pins psi at both ends as NUMBERS, so a word is admissible only if its net turning (the signed sum of its arc angles)
equals psi1 - psi0 to TURN_TOL; L*(rho) is the shortest admissible length, +inf where there is none, ties to the lower word index.

The searches.  F(v) = L*(rho(v)) - v T.  Tight (F(v_pref) > 0): the speed in [v_pref, v_hi], sides (F > 0, F <= 0), the result the
UPPER end of the last bracket.  Loose: the radius in a bracket grown by GROW from rho(v_pref), sides (L* - v T < 0, >= 0), the result
the LOWER end.  Both results are on the side where the path is no longer than v T.  L* can jump -- a word stops existing, or stops
being admissible -- and the upper end of a radius bracket can then be a path many times longer than v T (case 1 of
tests/nlp_guess_cases.py with its bounds: 4877 m for a budget of 168 m); the lower end never is.  Where L* is continuous the two
ends differ by the width of the last bracket, (b - a) / 64^ROUNDS.  ROUNDS = 3: the points of a round lie (b - a) / 64^r apart, so
from the fourth round on an evaluation within 1e-9 v T of zero -- where two machines may disagree on its sign -- stops being rare
and from the sixth it is certain; three rounds give the speed to 1e-5 m/s and the length to a fraction of a millimetre, far below
what the chords of a 0.1 s step leave, and keep every decision of the search away from rounding.
"""
import numpy as np

G_ACC = 9.81
TWO_PI = 2.0 * np.pi
WORDS = ('LSL', 'RSR', 'LSR', 'RSL', 'RLR', 'LRL')
# (sign of the first arc, of the middle segment (0: straight), of the last arc)
WORD_SIGNS = ((1, 0, 1), (-1, 0, -1), (1, 0, -1), (-1, 0, 1), (-1, 1, -1), (1, -1, 1))
FIT, SHORT, LOOSE, LOOSE_UNMET, LINE, INVALID = range(6)      # include/d2d.h D2D_GUESS_*
STATUS = ('FIT', 'SHORT', 'LOOSE', 'LOOSE_UNMET', 'LINE', 'INVALID')
KAPPA = 0.9               # D2D_GUESS_KAPPA: the fraction of the bank limit the arcs use
TURN_TOL = 1e-9           # D2D_GUESS_TURN_TOL
ROUNDS, SECTIONS = 3, 64  # D2D_GUESS_ROUNDS rounds of 64-section
GROW, GROW_MAX = 1.5, 24  # D2D_GUESS_GROW, D2D_GUESS_GROW_MAX: the bracket of the radius search

# scenario row columns (d2dhip.SC_*; tests/test_nlp_guess_cpu.py compares)
SC_X0, SC_X1, SC_VREF, SC_VSP, SC_KV, SC_WX, SC_WY, SC_PHIMAX, SC_VMIN, SC_VMAX = 0, 3, 6, 7, 8, 13, 14, 23, 24, 25


# The transcendentals go through these names so that floors() can move the result of one of them by one ulp (sqrt and fmod are
# correctly rounded on both sides and stay as they are).
TRANSCENDENTALS = ('sin', 'cos', 'tan', 'atan', 'atan2', 'acos')
_BUMP = [None, 0.0]


def _bumped(name, f):
    def g(*a):
        r = f(*a)
        return np.nextafter(r, _BUMP[1] * np.inf) if _BUMP[0] == name else r
    return g


_sin, _cos, _tan = _bumped('sin', np.sin), _bumped('cos', np.cos), _bumped('tan', np.tan)
_atan, _atan2, _acos = _bumped('atan', np.arctan), _bumped('atan2', np.arctan2), _bumped('acos', np.arccos)


def _mod2pi(x):
    r = np.fmod(x, TWO_PI)
    return np.where(r < 0.0, r + TWO_PI, r)


def words(p0, p1, rho):
    """The six words from pose p0 to pose p1 (x, y, psi) at the radii rho [n]: (length [6][n], +inf where the word does not exist
    or is not admissible; segment lengths seg [6][3][n])."""
    rho = np.atleast_1d(np.asarray(rho, float))
    n = rho.shape[0]
    s0, c0, s1, c1 = _sin(p0[2]), _cos(p0[2]), _sin(p1[2]), _cos(p1[2])
    dpsi = p1[2] - p0[2]
    length = np.full((6, n), np.inf)
    seg = np.zeros((6, 3, n))

    def put(w, ok, t, mid, q, net):
        ok = ok & (np.abs(net - dpsi) <= TURN_TOL)
        seg[w] = rho * t, mid, rho * q
        length[w] = np.where(ok, (seg[w, 0] + seg[w, 1]) + seg[w, 2], np.inf)

    for w, (a, b) in enumerate(((1, 1), (-1, -1), (1, -1), (-1, 1))):
        dx = (p1[0] - b * rho * s1) - (p0[0] - a * rho * s0)
        dy = (p1[1] + b * rho * c1) - (p0[1] + a * rho * c0)
        l2 = dx * dx + dy * dy
        gam = _atan2(dy, dx)
        if a == b:
            t, q = _mod2pi(a * (gam - p0[2])), _mod2pi(b * (p1[2] - gam))
            put(w, np.ones(n, bool), t, np.sqrt(l2), q, a * t + b * q)
            # the C C C word of the same centres: s = a, signs (s, -s, s)
            l = np.sqrt(l2)
            A = _acos(np.minimum(l / (4.0 * rho), 1.0))
            chi1 = gam + a * A + a * (0.5 * np.pi)
            chi2 = (gam + np.pi - a * A) + a * (0.5 * np.pi)
            t, m, q = _mod2pi(a * (chi1 - p0[2])), np.pi + 2.0 * A, _mod2pi(a * (p1[2] - chi2))
            put(5 if a > 0 else 4, l <= 4.0 * rho, t, rho * m, q, a * ((t - m) + q))
        else:
            p2 = l2 - 4.0 * rho * rho
            p = np.sqrt(np.maximum(p2, 0.0))
            chi = gam + a * _atan2(2.0 * rho, p)
            t, q = _mod2pi(a * (chi - p0[2])), _mod2pi(b * (p1[2] - chi))
            put(w, p2 >= 0.0, t, p, q, a * t + b * q)
    return length, seg


def lstar(p0, p1, rho):
    """L*(rho) [n], its word [n] and the second-shortest admissible length [n] (+inf: none)."""
    length, _ = words(p0, p1, rho)
    w = np.argmin(length, 0)                       # the first minimum: ties to the lower word index
    best = np.take_along_axis(length, w[None], 0)[0]
    rest = length.copy()
    np.put_along_axis(rest, w[None], np.inf, 0)
    return best, w, rest.min(0)


def radius(v, phi_max, kappa):
    return v * v / (G_ACC * _tan(kappa * phi_max))


def _section(f, a, b, side_of):
    """ROUNDS rounds of SECTIONS-section on [a, b] -> the last bracket.  side_of(f(x)) is True on the lower end's side; the lower end
    of a bracket has side True and the upper end side False BY THE INVARIANT (they are not asked again).  A round evaluates the
    points a + (b - a) k / 64, k = 1 .. 63, and takes the first k from the lower end with side(k) and not side(k + 1)."""
    for _ in range(ROUNDS):
        k = np.arange(SECTIONS + 1)
        x = a + (b - a) * (k / float(SECTIONS))
        x[SECTIONS] = b
        side = side_of(f(x[1:SECTIONS]))
        side = np.concatenate([[True], side, [False]])
        first = int(np.flatnonzero(side[:-1] & ~side[1:])[0])
        a, b = x[first], x[first + 1]
    return a, b


def guess_one(row, N, h, bounds=None, v_pref=None, kappa=KAPPA, trace=None):
    """One problem.  row: the scenario row; bounds: None or (phi_lo, phi_hi, psi_lo, psi_hi); v_pref: None or a number.
    -> (W [5][N] or None when refused, dict(status, word, v, rho, L, t_nat)).
    trace: a list that receives ('F', |F| / (v T)) of every search evaluation and ('margin', (second - best) / best) at the bracket
    ends and at the result (tests/test_nlp_guess_cpu.py: determinacy)."""
    row = np.asarray(row, float)
    nan = float('nan')
    refused = dict(status=INVALID, word=-1, v=nan, rho=nan, L=nan, t_nat=nan)
    p0, p1 = row[SC_X0:SC_X0 + 3].copy(), row[SC_X1:SC_X1 + 3].copy()
    wx, wy = row[SC_WX], row[SC_WY]                  # the drift of the kernel's equalities: x' = v cos psi + SC_WX
    v_lo, v_hi, phi_max = row[SC_VMIN], row[SC_VMAX], row[SC_PHIMAX]
    read = [*p0, *p1, wx, wy, v_lo, v_hi, phi_max]
    if bounds is not None:
        read += [bounds[0], bounds[1]]
        if bounds[0] < bounds[1]:
            phi_max = min(abs(bounds[0]), abs(bounds[1]))
    if v_pref is None:
        read += [row[SC_KV], row[SC_VSP], row[SC_VREF]]
        vp = row[SC_VSP] if row[SC_KV] > 0.0 else (row[SC_VREF] if row[SC_VREF] > 0.0 else 0.5 * (v_lo + v_hi))
    else:
        read += [v_pref]
        vp = float(v_pref)
    if (not np.all(np.isfinite(read)) or not v_lo > 0.0 or v_lo > v_hi or not (0.0 < phi_max < 0.5 * np.pi)
            or N < 2 or not h > 0.0 or not np.isfinite(h)):
        return None, refused
    vp = min(max(vp, v_lo), v_hi)
    T = (N - 1) * h
    q1 = np.array([p1[0] - wx * T, p1[1] - wy * T, p1[2]])       # the end pose in the air frame

    def note(kind, val):
        if trace is not None:
            trace.extend((kind, float(x)) for x in np.atleast_1d(val))

    def L_of_rho(rho):
        best, _, second = lstar(p0, q1, rho)
        return best, second

    def F_of_v(v):                               # L*(rho(v)) - v T
        v = np.atleast_1d(v)
        best, _ = L_of_rho(radius(v, phi_max, kappa))
        f = best - v * T
        note('F', np.abs(f) / (v * T))
        return f

    def G_of_rho(rho):                           # L*(rho) - v_pref T
        best, _ = L_of_rho(np.atleast_1d(rho))
        f = best - vp * T
        note('F', np.abs(f) / (vp * T))
        return f

    def margin(rho):
        best, second = L_of_rho(np.atleast_1d(rho))
        if np.isfinite(best[0]) and best[0] > 0.0:
            note('margin', (second - best) / best)

    rho0 = float(radius(vp, phi_max, kappa))
    L0 = float(L_of_rho(rho0)[0][0])
    t_nat = L0 / vp if np.isfinite(L0) else nan
    line = abs(p1[2] - p0[2]) >= TWO_PI or not np.isfinite(L0) or L0 == 0.0
    v, rho, status = vp, rho0, LINE
    if not line:
        margin(rho0)
        if F_of_v(vp)[0] > 0.0:               # tight: a faster aircraft, v in [v_pref, v_hi]
            margin(radius(v_hi, phi_max, kappa))
            if F_of_v(v_hi)[0] > 0.0:
                v, status = v_hi, SHORT
            else:
                _, v = _section(F_of_v, vp, v_hi, lambda f: f > 0.0)
                status = FIT
            rho = float(radius(v, phi_max, kappa))
        else:                                        # loose: v_pref on wider turns, rho >= rho(v_pref)
            lo = hi = rho0
            status = LOOSE_UNMET
            for _ in range(GROW_MAX):
                lo, hi = hi, hi * GROW
                if G_of_rho(hi)[0] >= 0.0:
                    status = LOOSE
                    break
            margin(hi)
            rho = hi
            if status == LOOSE:
                margin(lo)
                rho, _ = _section(G_of_rho, lo, hi, lambda f: f < 0.0)     # the LOWER end: L* < v T, see the module docstring
        margin(rho)
    W = np.zeros((5, N))
    frac = np.arange(N) / float(N - 1)
    L = nan
    word = -1
    if not line:
        length, seg = words(p0, q1, rho)
        word = int(np.argmin(length[:, 0]))
        L = float(length[word, 0])
        line = not np.isfinite(L) or L == 0.0        # (a search that ended where no word is admissible)
    if line:
        status, word, v, rho = LINE, -1, vp, float('inf')
        L = float(np.sqrt((p1[0] - p0[0]) ** 2 + (p1[1] - p0[1]) ** 2))
        for c in range(3):
            W[c] = p0[c] + (p1[c] - p0[c]) * frac
        W[4] = v
    else:
        l1, l2, l3 = seg[word, :, 0]
        signs = WORD_SIGNS[word]
        sig = L * frac
        sig[N - 1] = L

        def advance(P, s, d):
            if s == 0:
                return P[0] + d * _cos(P[2]), P[1] + d * _sin(P[2]), P[2] + 0.0 * d
            psi = P[2] + s * (d / rho)
            return P[0] + s * rho * (_sin(psi) - _sin(P[2])), P[1] - s * rho * (_cos(psi) - _cos(P[2])), psi

        P0 = (p0[0], p0[1], p0[2])
        P1 = advance(P0, signs[0], l1)
        P2 = advance(P1, signs[1], l2)
        which = np.where(sig <= l1, 0, np.where(sig <= l1 + l2, 1, 2))       # a node on a junction belongs to the earlier segment
        bank = _atan(v * v / (G_ACC * rho))
        for k, (P, start) in enumerate(((P0, 0.0), (P1, l1), (P2, l1 + l2))):
            x, y, psi = advance(P, signs[k], sig - start)
            m = which == k
            W[0, m], W[1, m], W[2, m], W[3, m] = x[m], y[m], psi[m], signs[k] * bank
        t = np.arange(N) * h
        W[0] += wx * t
        W[1] += wy * t
        W[4] = v
    W[:3, 0], W[:3, N - 1] = p0, p1                  # the pinned ends, as numbers
    return W, dict(status=status, word=word, v=float(v), rho=float(rho), L=L, t_nat=t_nat)


def guess(rows, N, h, bounds=None, v_pref=None, kappa=KAPPA, W=None):
    """The batch: rows [B][stride], bounds [B][4] or None, v_pref [B] or None.  W [B][5][N]: a refused row keeps its values (zeros if
    W is None).  -> (W, dict of arrays status, word int32 [B]; v, rho, L, t_nat [B])."""
    rows = np.asarray(rows, float)
    B = rows.shape[0]
    if not 0.0 < kappa <= 1.0:
        raise ValueError(f'kappa = {kappa} outside (0, 1]')
    W = np.zeros((B, 5, N)) if W is None else W
    out = dict(status=np.zeros(B, np.int32), word=np.zeros(B, np.int32), v=np.zeros(B), rho=np.zeros(B), L=np.zeros(B), t_nat=np.zeros(B))
    for b in range(B):
        Wb, o = guess_one(rows[b], N, h, None if bounds is None else bounds[b], None if v_pref is None else v_pref[b], kappa)
        if Wb is not None:
            W[b] = Wb
        for k, val in o.items():
            out[k][b] = val
    return W, out


QUANTITIES = ('x', 'y', 'psi', 'phi', 'vnode', 'v', 'rho', 'L', 't_nat')


def _quantities(W, o):
    return [W[0], W[1], W[2], W[3], W[4]] + [np.array([o[k]]) for k in ('v', 'rho', 'L', 't_nat')]


def difference(Wa, oa, Wb, ob):
    """Largest |a - b| per quantity of QUANTITIES (0 where both are the same non-finite value)."""
    d = []
    for a, b in zip(_quantities(Wa, oa), _quantities(Wb, ob)):
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        with np.errstate(invalid='ignore'):
            d.append(float(np.max(np.where(same, 0.0, np.abs(a - b)))))
    return np.array(d)


def floors(row, N, h, bounds=None, v_pref=None, kappa=KAPPA):
    """The statement's own floor for one problem: the largest change of each quantity of QUANTITIES when one of the six end-pose
    entries moves by one ulp, either way, and when the result of one transcendental (TRANSCENDENTALS) moves by one ulp, either way.
    A perturbation that changes status or word raises: such a problem is not determined and is no parity case."""
    row = np.asarray(row, float)
    W0, o0 = guess_one(row, N, h, bounds, v_pref, kappa)
    f = np.zeros(len(QUANTITIES))
    if W0 is None:
        return f
    for sign in (-1.0, 1.0):
        for c in (SC_X0, SC_X0 + 1, SC_X0 + 2, SC_X1, SC_X1 + 1, SC_X1 + 2):
            r = row.copy()
            r[c] = np.nextafter(r[c], sign * np.inf)
            W1, o1 = guess_one(r, N, h, bounds, v_pref, kappa)
            assert (o1['status'], o1['word']) == (o0['status'], o0['word']), (c, sign, o0, o1)
            W1[:3, 0], W1[:3, N - 1] = W0[:3, 0], W0[:3, N - 1]         # (the pinned ends move with the input: not an error of the rule)
            f = np.maximum(f, difference(W0, o0, W1, o1))
        for name in TRANSCENDENTALS:
            _BUMP[:] = [name, sign]
            try:
                W1, o1 = guess_one(row, N, h, bounds, v_pref, kappa)
            finally:
                _BUMP[:] = [None, 0.0]
            assert (o1['status'], o1['word']) == (o0['status'], o0['word']), (name, sign, o0, o1)
            f = np.maximum(f, difference(W0, o0, W1, o1))
    return f
