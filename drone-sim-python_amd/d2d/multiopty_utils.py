"""Mirror of src/d2d/multiopty_utils.py: the aircraft set and the multi-aircraft cost
plug-ins (same protocol as d2d.opty_utils; slices are lists, one per aircraft)."""
import numpy as np

import d2d.opty_utils as d2ou


class AircraftSet:
    def __init__(self, n=2):
        self.st = d2ou._Sym('t')
        self.nb_aicraft = n                    # (sic) the reference's attribute name
        self.aircraft = [d2ou.Aircraft(self.st, i) for i in range(n)]
        self._state_symbols = tuple(s for ac in self.aircraft for s in ac._state_symbols)
        self._input_symbols = tuple(s for ac in self.aircraft for s in ac._input_symbols)

    def get_eom(self, wind, g=9.81):
        """The stacked model of all aircraft (src/d2d/multiopty_utils.py:25-26)."""
        return d2ou.Eom(wind.sample_sym(self.st, None, None), g, tuple(ac._id for ac in self.aircraft))


def _scale(_p):
    return _p.obj_scale / _p.num_nodes / _p.acs.nb_aicraft


class CostNull:
    def cost(self, free, _p):
        return 0.

    def cost_grad(self, free, _p):
        return np.zeros_like(free)


class CostInput:
    """scale/N/n_ac * (kv sum (v-vsp)^2 + kphi sum phi^2) over all aircraft (src/d2d/multiopty_utils.py:56-71)."""

    def __init__(self, vsp=10., kv=1., kphi=1.):
        self.vsp, self.kv, self.kphi = vsp, kv, kphi

    def cost(self, free, _p):
        sp = sum(np.sum(free[s] ** 2) for s in _p._slice_phi)
        sv = sum(np.sum((free[s] - self.vsp) ** 2) for s in _p._slice_v)
        return _scale(_p) * (self.kv * sv + self.kphi * sp)

    def cost_grad(self, free, _p):
        g = np.zeros_like(free)
        for s in _p._slice_phi:
            g[s] = self.kphi * 2 * free[s]
        for s in _p._slice_v:
            g[s] = self.kv * 2 * (free[s] - self.vsp)
        return g * _scale(_p)


class CostAirvel(CostInput):
    """(src/d2d/multiopty_utils.py:33-43)."""

    def __init__(self, vsp=10.):
        CostInput.__init__(self, vsp, 1., 0.)


class CostBank(CostInput):
    """(src/d2d/multiopty_utils.py:45-54)."""

    def __init__(self):
        CostInput.__init__(self, 0., 0., 1.)


class CostObstacle:
    """Obstacle penalty on aircraft 0 only, scale without 1/n_ac (src/d2d/multiopty_utils.py:74-106)."""

    def __init__(self, c=(0, 0), r=10., kind=0):
        self.c, self.r, self.kind, self.k = c, r, kind, 2

    def _d(self, free, _p):
        return free[_p._slice_x[0]] - self.c[0], free[_p._slice_y[0]] - self.c[1]

    def cost(self, free, _p):
        return _p.obj_scale / _p.num_nodes * np.sum(d2ou._obstacle_field(*self._d(free, _p), self.r, self.kind, self.k))

    def cost_grad(self, free, _p):
        dx, dy = self._d(free, _p)
        e = d2ou._obstacle_field(dx, dy, self.r, self.kind, self.k)
        g = np.zeros_like(free)
        g[_p._slice_x[0]] = _p.obj_scale / _p.num_nodes * -2. * dx * e
        g[_p._slice_y[0]] = _p.obj_scale / _p.num_nodes * -2. * dy * e
        return g


class CostObstacles:
    def __init__(self, obss, kind=0):
        self.obss = [CostObstacle(c=(o[0], o[1]), r=o[2], kind=kind) for o in obss]

    def cost(self, free, _p):
        return np.sum([c.cost(free, _p) for c in self.obss])

    def cost_grad(self, free, _p):
        return np.sum([c.cost_grad(free, _p) for c in self.obss], axis=0)


def collision_pairs(pairs, n):
    """The unordered pairs (i, j), i < j, that a `pairs` argument selects among n aircraft: None -> the reference's pair (0, 1)
    (src/d2d/multiopty_utils.py:124-125), 'all' -> every pair, an iterable of (i, j) -> those.  ValueError for i == j, an index
    outside 0 .. n-1 or a repeated pair."""
    if pairs is None:
        return [(0, 1)]
    if isinstance(pairs, str):
        if pairs != 'all':
            raise ValueError(f"pairs: None, 'all' or an iterable of (i, j), not {pairs!r}")
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    out = []
    for p in pairs:
        try:
            i, j = p
            ok = int(i) == i and int(j) == j
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'pairs: {p!r} is not a pair of aircraft indices')
        i, j = int(i), int(j)
        if i == j:
            raise ValueError(f'pairs: aircraft {i} paired with itself')
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError(f'pairs: ({i}, {j}) names an aircraft outside 0 .. {n - 1}')
        q = (min(i, j), max(i, j))
        if q in out:
            raise ValueError(f'pairs: {q} given twice')
        out.append(q)
    return out


def pair_masks(pairs, n):
    """Partner set of each of n aircraft (bit j: coupled with aircraft j -- D2D_SC_PMASK) for the pairs of collision_pairs."""
    masks = [0] * n
    for i, j in pairs:
        masks[i] |= 1 << j
        masks[j] |= 1 << i
    return masks


def default_pair_masks(dsc, n_ac, on):
    """The reference's pair (0, 1) as partner sets, for the entries that read them (d2d_nlp_solve_groups_moving / _via): D2D_SC_PMASK
    of the scenario rows dsc [R * n_ac][SCEN_STRIDE] (in place) becomes 0b10 on aircraft 0 and 0b01 on aircraft 1 of every scenario
    where `on` holds (True, or a boolean tensor [R]) and 0 where it does not."""
    from d2dhip import SC_PMASK
    dsc[0::n_ac, SC_PMASK] = on * 2.0
    dsc[1::n_ac, SC_PMASK] = on * 1.0


class CostCollision:
    """Gaussian proximity penalty between aircraft 0 and 1 (src/d2d/multiopty_utils.py:120-153).  pairs: None -- that pair, as in
    the reference; 'all' -- every unordered pair of the planner's aircraft; an iterable of (i, j) -- those pairs.  The same term
    for every selected pair, each pair once, scale obj_scale / num_nodes."""

    def __init__(self, r=3., k=2., pairs=None):
        self.r, self.k, self.pairs = r, k, pairs

    def _pairs(self, _p):
        return collision_pairs(self.pairs, len(_p._slice_x))

    def _d(self, free, _p, i=0, j=1):
        return free[_p._slice_x[i]] - free[_p._slice_x[j]], free[_p._slice_y[i]] - free[_p._slice_y[j]]

    def cost(self, free, _p):
        if self.pairs is None:
            dx, dy = self._d(free, _p)
            return _p.obj_scale / _p.num_nodes * np.sum(d2ou._obstacle_field(dx, dy, self.r, 1, self.k))
        return _p.obj_scale / _p.num_nodes * sum(np.sum(d2ou._obstacle_field(*self._d(free, _p, i, j), self.r, 1, self.k))
                                                 for i, j in self._pairs(_p))

    def cost_grad(self, free, _p):
        f = _p.obj_scale / _p.num_nodes
        g = np.zeros_like(free)
        if self.pairs is None:
            dx, dy = self._d(free, _p)
            e = d2ou._obstacle_field(dx, dy, self.r, 1, self.k)
            g[_p._slice_x[0]], g[_p._slice_y[0]] = f * -2. * dx * e, f * -2. * dy * e
            g[_p._slice_x[1]], g[_p._slice_y[1]] = f * 2. * dx * e, f * 2. * dy * e
            return g
        for i, j in self._pairs(_p):
            dx, dy = self._d(free, _p, i, j)
            e = d2ou._obstacle_field(dx, dy, self.r, 1, self.k)
            g[_p._slice_x[i]] += f * -2. * dx * e; g[_p._slice_y[i]] += f * -2. * dy * e
            g[_p._slice_x[j]] += f * 2. * dx * e; g[_p._slice_y[j]] += f * 2. * dy * e
        return g


class CostComposit:
    """CostInput [+ kobs * obstacles] [+ kcol * collision]; a NaN weight switches a term off
    (src/d2d/multiopty_utils.py:156-174).  col_pairs: CostCollision's `pairs`."""

    def __init__(self, kvel=1., kbank=1., kobs=float('Nan'), kcol=float('NaN'), vsp=10., obss=[], obs_kind=0, rcol=3., col_pairs=None):
        self.kvel, self.kbank, self.kobs, self.kcol = kvel, kbank, kobs, kcol
        self.vsp, self.obss, self.obs_kind, self.rcol = vsp, obss, obs_kind, rcol
        self.ci = CostInput(vsp, kvel, kbank)
        self.cobs = CostObstacles(obss, obs_kind)      # always constructed, as in the reference (:160-161)
        self.col_pairs = col_pairs                     # CostCollision(pairs=): None = the reference's pair (0, 1)
        self.ccol = CostCollision(r=rcol, pairs=col_pairs)

    def _extra(self):
        return [(k, c) for k, c in ((self.kobs, self.cobs), (self.kcol, self.ccol)) if not np.isnan(k)]

    def cost(self, free, _p):
        return self.ci.cost(free, _p) + sum(k * c.cost(free, _p) for k, c in self._extra())

    def cost_grad(self, free, _p):
        return self.ci.cost_grad(free, _p) + sum(k * c.cost_grad(free, _p) for k, c in self._extra())
