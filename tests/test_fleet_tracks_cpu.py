"""CPU: the statement of d2d_fleet_tracks (tests/fleet_tracks_ref.py) on hand-made cases whose answers are written out here, and the
host logic of full_sim.deconflict_plans / plan_batch(deconflict=) with a stub context that records its calls (torch on the CPU)."""
import os
import re

import numpy as np
import pytest

import fleet_tracks_ref as FT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hist(paths):
    """paths: one list of (x, y) per aircraft, all of one length -> X [n_rows][5][N]."""
    P = np.asarray(paths, dtype=np.float64)
    X = np.zeros((P.shape[1], 5, P.shape[0]))
    X[:, 0], X[:, 1] = P[:, :, 0].T, P[:, :, 1].T
    return X


def test_abi_and_constants():
    import d2dhip
    hdr = open(os.path.join(ROOT, 'include', 'd2d.h')).read()
    assert int(re.search(r'#define D2D_VERSION (\d+)', hdr).group(1)) >= 125
    assert int(re.search(r'#define D2D_TRACKS_SHORT (\d+)', hdr).group(1)) == d2dhip.TRACKS_SHORT == FT.SHORT
    assert 'd2d_fleet_tracks' in d2dhip.EXPORTS and 'd2d_fleet_tracks_workspace' in d2dhip.EXPORTS
    assert [k for k, _ in d2dhip.TracksOut._fields_] == re.search(r'typedef struct \{([^}]*)\} d2d_tracks_out', hdr).group(1).replace('*', ' ').replace(
        'double', ' ').replace('int32_t', ' ').replace(';', ' ').split()


def test_two_crossing_aircraft():
    """Formation 0 flies east along y = 0, formation 1 north along x = 0; they pass between rows 1 and 2.  Seen from aircraft 1:
    p0 = (-2, 1) at row 1, p1 = (0, -1) at row 2, d = (2, -2), s* = 6 / 8, q = (-0.5, -0.5): d^2 = 0.5 at u = 1.75."""
    X = _hist([[(2 * i - 4, 0) for i in range(5)], [(0, 2 * i - 3) for i in range(5)]])
    o = FT.tracks(X, 1, 0.5, 4.0, 3.0, 2.5, n_mov=2, n_knot=3, kind=1, t0=10.0)
    assert list(o['n_conf']) == [0, 1] and list(o['status']) == [0, 0]
    assert o['partner'].tolist() == [[-1, -1], [0, -1]]
    assert o['part_dist'][1, 0] == np.sqrt(0.5) and o['part_time'][1, 0] == 1.75 * 0.5 and np.isinf(o['part_dist'][0]).all()
    # knots of formation 1 at its rows 0, 2, 4: times 10 + g / 2, the partner's own positions there
    assert o['knots'][1, 0].tolist() == [[10.0, -4.0, 0.0], [11.0, 0.0, 0.0], [12.0, 4.0, 0.0]]
    assert o['knots'][1, 1].tolist() == [[10.0, 0.0, 0.0], [11.0, 0.0, 0.0], [12.0, 0.0, 0.0]]          # the absent slot's dummy track
    assert o['disc'].tolist() == [[[0.0, 1.0], [0.0, 1.0]], [[2.5, 1.0], [0.0, 1.0]]]
    assert o['chord_err'][1].tolist() == [0.0, 0.0]           # a straight path at constant speed is its own chord
    # the other way round: formation 1 outranks formation 0
    o = FT.tracks(X, 1, 0.5, 4.0, 3.0, 2.5, prio=[1, 0], n_mov=2, n_knot=3)
    assert o['partner'].tolist() == [[1, -1], [-1, -1]] and list(o['n_conf']) == [1, 0]
    assert o['part_dist'][0, 0] == np.sqrt(0.5) and o['part_time'][0, 0] == 1.75 * 0.5


def test_a_tie_in_distance_is_broken_by_time_and_then_by_index():
    """Aircraft 3 stands at the origin.  Aircraft 0 comes to 3 m at row 2, aircraft 1 and 2 at row 1 (and stay): all keys have
    d^2 = 9; the order is (9, 1, B = 1), (9, 1, B = 2), (9, 2, B = 0)."""
    X = _hist([[(5, 0), (4, 0), (3, 0)], [(0, 4), (0, 3), (0, 3)], [(-4, 0), (-3, 0), (-3, 0)], [(0, 0)] * 3])
    o = FT.tracks(X, 1, 1.0, 3.5, 1.5, 1.0, n_mov=3, n_knot=2, full=True)
    assert o['partner'][3].tolist() == [1, 2, 0] and o['n_conf'][3] == 3
    assert o['part_dist'][3].tolist() == [3.0, 3.0, 3.0] and o['part_time'][3].tolist() == [1.0, 1.0, 2.0]
    assert o['members'][3] == [(9.0, 1.0, 3, 1), (9.0, 1.0, 3, 2), (9.0, 2.0, 3, 0)]
    # two slots: the third partner is cut and n_conf says so
    o = FT.tracks(X, 1, 1.0, 3.5, 1.5, 1.0, n_mov=2, n_knot=2)
    assert o['partner'][3].tolist() == [1, 2] and o['n_conf'][3] == 3
    # the same partner seen by two aircraft of one formation at the same distance and time: the smaller A keys it, one entry
    X = _hist([[(0, 3), (0, 3)], [(50, 50), (50, 50)], [(0, 0), (0, 0)], [(0, 6), (0, 6)]])
    o = FT.tracks(X, 2, 1.0, 3.5, 1.5, 1.0, n_mov=2, n_knot=2, full=True)
    assert o['members'][1] == [(9.0, 0.0, 2, 0)] and o['partner'][1].tolist() == [0, -1]


def test_only_the_lower_side_of_a_pair_lists_its_partner():
    """Three formations in a row, 2 m apart, standing still: each lists those that outrank it, nearest first; equal prio falls back to
    the formation index; worlds do not see each other."""
    X = _hist([[(0, 0)] * 2, [(2, 0)] * 2, [(4, 0)] * 2])
    o = FT.tracks(X, 1, 1.0, 5.0, 1.0, 1.0, n_mov=2, n_knot=2)
    assert o['partner'].tolist() == [[-1, -1], [0, -1], [1, 0]]
    o = FT.tracks(X, 1, 1.0, 5.0, 1.0, 1.0, prio=[7, 7, 1], n_mov=2, n_knot=2)
    assert o['partner'].tolist() == [[2, -1], [0, 2], [-1, -1]]           # 2 outranks both; between 0 and 1 the index decides
    o = FT.tracks(X, 1, 1.0, 5.0, 1.0, 1.0, world=[0, 1, 0], n_mov=2, n_knot=2)
    assert o['partner'].tolist() == [[-1, -1], [-1, -1], [0, -1]]


def test_knots_clamp_chord_error_and_short_windows():
    """The partner flies (0,0) (1,1) (2,0) (3,1) (4,0) from global row 1; formation 1 stands at (2, 0.5) over global rows 0 .. 4.  Two
    knots: rows 0 and 4 -- the partner is held at its first row before its window, so the track runs (0,0) -> (3,1) and its chord error
    is taken over the partner's own rows 1 .. 4: row 3 (partner (2, 0), track (2.25, 0.75)) gives sqrt(0.0625 + 0.5625)."""
    X = _hist([[(0, 0), (1, 1), (2, 0), (3, 1), (4, 0)], [(2, 0.5)] * 5])
    kw = dict(rows=[5, 5], row0=[1, 0], n_mov=1, t0=0.0)
    o = FT.tracks(X, 1, 1.0, 3.0, 1.5, 1.0, n_knot=2, **kw)
    assert o['knots'][1, 0].tolist() == [[0.0, 0.0, 0.0], [4.0, 3.0, 1.0]] and o['partner'][1, 0] == 0
    e2 = [0.75 ** 2 + 0.25 ** 2, 0.5 ** 2 + 0.5 ** 2, 0.25 ** 2 + 0.75 ** 2, 0.0]          # global rows 1 .. 4 (every term exact)
    assert o['chord_err'][1, 0] == np.sqrt(max(e2)) == np.sqrt(0.625)
    # five knots, one per row: nothing is given away; the partner's last rows are outside formation 1's window and are not looked at
    o = FT.tracks(X, 1, 1.0, 3.0, 1.5, 1.0, n_knot=5, **kw)
    assert o['chord_err'][1, 0] == 0.0 and o['knots'][1, 0, :, 1].tolist() == [0.0, 0.0, 1.0, 2.0, 3.0]
    # six knots do not fit into five rows: SHORT -- but the formation is still seen by the one it outranks
    o = FT.tracks(X, 1, 1.0, 3.0, 1.5, 1.0, n_knot=6, prio=[1, 0], **kw)
    assert list(o['status']) == [FT.SHORT, FT.SHORT] and list(o['n_conf']) == [-1, -1]
    o = FT.tracks(X, 1, 1.0, 3.0, 1.5, 1.0, n_knot=5, prio=[1, 0], rows=[5, 4], row0=[1, 0], n_mov=1)
    assert list(o['status']) == [0, FT.SHORT] and o['partner'].tolist() == [[1], [-1]]
    assert o['knots'][1, 0, :, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and np.isnan(o['part_dist'][1, 0])


# ---- the loop's host logic, with a stub context ------------------------------------------------------------------------------------
class _Stub:
    """Records every call; fleet_tracks plays a script of (n_conf, partner) per round; the solves add 1 to the plans they are given
    and report the scripted status."""

    def __init__(self, script, R, n_mov, status=None):
        import torch
        self.torch, self.script, self.R, self.n_mov, self.status = torch, list(script), R, n_mov, status or {}
        self.calls, self.device = [], torch.device('cpu')

    def dev(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a))

    def fleet_tracks(self, X, n_ac, dt_row, d_look, step_max, r_disc, n_knot=32, n_mov=8, **kw):
        t = self.torch
        n_conf, partner = self.script.pop(0)
        self.calls.append(('fleet_tracks', dict(X=X.clone(), n_ac=n_ac, dt_row=dt_row, d_look=d_look, step_max=step_max, r_disc=r_disc, **kw)))
        partner = t.tensor(partner, dtype=t.int32)
        knots = t.zeros(self.R, n_mov, n_knot, 3, dtype=t.float64) + t.arange(self.R, dtype=t.float64)[:, None, None, None]
        disc = t.zeros(self.R, n_mov, 2, dtype=t.float64)
        disc[:, :, 0] = t.where(partner >= 0, r_disc, 0.0)
        return dict(knots=knots, disc=disc, partner=partner, chord_err=t.where(partner >= 0, 0.25, 0.0).to(t.float64),
                    n_conf=t.tensor(n_conf, dtype=t.int32), status=t.zeros(self.R, dtype=t.int32))

    def _solve(self, name, scen, W, h, n_ac, **kw):
        t = self.torch
        self.calls.append((name, dict(scen=scen.clone(), W_in=W.clone(), h=h, n_ac=n_ac, **kw)))
        W += 1.0
        forms = kw['knots'][:, 0, 0, 0].to(t.int64)                # the stub's knots carry the formation index
        st = t.tensor([self.status.get(int(f), 1) for f in forms], dtype=t.int32).repeat_interleave(n_ac)
        B = W.shape[0]
        return dict(cost=t.ones(B, dtype=t.float64), feas=t.zeros(B, dtype=t.float64), status=st, iters=t.ones(B, dtype=t.int32))

    def nlp_solve_groups_moving(self, scen, W, h, n_ac, **kw):
        return self._solve('nlp_solve_groups_moving', scen, W, h, n_ac, **kw)

    def nlp_solve_moving(self, scen, W, h, **kw):
        return self._solve('nlp_solve_moving', scen, W, h, 1, **kw)

    def nlp_solve_groups(self, scen, W, h, n_ac=None, **kw):
        self.calls.append(('nlp_solve_groups', dict(n_ac=n_ac)))
        return dict(cost=None, feas=None, status=None, iters=None)

    def fleet_audit(self, X, n_ac, dt_row, d_look, step_max, d_safe=0.0, **kw):
        t = self.torch
        self.calls.append(('fleet_audit', dict(X=X.clone(), d_safe=d_safe, **kw)))
        near = t.full((X.shape[2],), 9.0, dtype=t.float64)
        near[-1] = 1.0
        return dict(near_dist=near, near_partner=t.zeros(X.shape[2], dtype=t.int32))


def _plans(R, n_ac, N=6):
    import torch
    import d2dhip
    W = torch.arange(R * n_ac, dtype=torch.float64)[:, None, None] * 100.0 + torch.zeros(R * n_ac, 5, N, dtype=torch.float64)
    scen = torch.zeros(R * n_ac, d2dhip.SCEN_STRIDE, dtype=torch.float64)
    scen[:, d2dhip.SC_VMAX] = 14.0
    scen[:, 0] = torch.arange(R * n_ac, dtype=torch.float64)                          # a tag to follow the gather by
    return scen, W


SCRIPT = [([0, 1, 0, 2], [[-1, -1], [0, -1], [-1, -1], [2, 4]])] * 3      # 1 gives way to 0; 3 to 1 and 2


def test_loop_resolves_only_what_can_have_changed_and_scatters_back():
    import full_sim
    R, n_ac = 4, 2
    scen, W = _plans(R, n_ac)
    W0 = W.clone()
    ctx = _Stub(SCRIPT, R, 2)
    Wr, info = full_sim.deconflict_plans(ctx, scen, W, 0.1, n_ac, row0=[0, 3, 0, 5], d_sep=4.0, margin=1.0, d_look=30.0, n_knot=4, n_mov=2, t0=2.0,
                                         max_sweeps=7)
    assert Wr is W and info['rounds'] == 2 and info['replanned'] == [2, 1]
    names = [c[0] for c in ctx.calls]
    assert names == ['fleet_tracks', 'nlp_solve_groups_moving', 'fleet_tracks', 'nlp_solve_groups_moving', 'fleet_tracks', 'fleet_audit']
    s1, s2 = ctx.calls[1][1], ctx.calls[3][1]
    # round 1: formations 1 and 3, their rows, plans, tables and start times t0 + row0 h; the radius carries the chord error
    assert s1['scen'][:, 0].tolist() == [2.0, 3.0, 6.0, 7.0] and s1['W_in'][:, 0, 0].tolist() == [200.0, 300.0, 600.0, 700.0]
    assert s1['knots'][:, 0, 0, 0].tolist() == [1.0, 3.0] and s1['t_start'].tolist() == [2.0 + 3 * 0.1, 2.0 + 5 * 0.1]
    assert s1['disc'][:, :, 0].tolist() == [[5.25, 0.0], [5.25, 5.25]] and s1['max_sweeps'] == 7 and s1['field'] is None
    # round 2: formation 1's partner (formation 0) did not move and its set is the same: skipped; formation 3's partner 1 moved
    assert s2['scen'][:, 0].tolist() == [6.0, 7.0] and s2['W_in'][:, 0, 0].tolist() == [601.0, 701.0]
    # round 3 finds nothing to do: formation 1 did not move in round 2
    assert (W - W0)[:, 0, 0].tolist() == [0, 0, 1, 1, 0, 0, 2, 2]
    # every fleet_tracks call saw the current plans as a history [N][5][R n_ac] with dt_row = h
    assert ctx.calls[2][1]['X'].shape == (6, 5, 8) and ctx.calls[2][1]['X'][0, 0].tolist() == [0, 100, 201, 301, 400, 500, 601, 701]
    assert ctx.calls[0][1]['dt_row'] == 0.1 and ctx.calls[0][1]['r_disc'] == 5.0 and ctx.calls[0][1]['t0'] == 2.0
    assert abs(ctx.calls[0][1]['step_max'] - 1.05 * 0.1 * 14.0) < 1e-12
    assert ctx.calls[-1][1]['d_safe'] == 4.0 and info['unresolved'] == [3] and info['not_converged'] == [] and info['truncated'] is False
    assert info['audit']['near_dist'][-1] == 1.0


def test_loop_keeps_the_plan_of_a_solve_that_did_not_converge_and_stops_at_max_rounds():
    import full_sim
    R, n_ac = 4, 1
    scen, W = _plans(R, n_ac)
    W0 = W.clone()
    script = [([0, 1, 0, 3], [[-1, -1], [0, -1], [-1, -1], [1, 2]])] * 2      # n_conf = n_mov + 1 = 3: truncated
    ctx = _Stub(script, R, 2, status={1: 2})
    _, info = full_sim.deconflict_plans(ctx, scen, W, 0.1, n_ac, d_sep=4.0, margin=1.0, d_look=30.0, n_knot=4, n_mov=2, max_rounds=1)
    assert [c[0] for c in ctx.calls] == ['fleet_tracks', 'nlp_solve_moving', 'fleet_audit']          # n_ac = 1: the single entry
    assert (W - W0)[:, 0, 0].tolist() == [0, 0, 0, 1] and info['not_converged'] == [1] and info['truncated'] is True and info['rounds'] == 1
    # nothing in conflict: no solve at all
    ctx = _Stub([([0, 0, 0, 0], [[-1, -1]] * 4)], R, 2)
    _, info = full_sim.deconflict_plans(ctx, scen, W, 0.1, n_ac, d_sep=4.0, margin=1.0, d_look=30.0, n_knot=4, n_mov=2)
    assert [c[0] for c in ctx.calls] == ['fleet_tracks', 'fleet_audit'] and info['rounds'] == 0 and info['replanned'] == []


def test_plan_batch_refusals_by_name_and_the_default_makes_no_new_call(monkeypatch):
    import torch
    import d2dhip
    import full_sim
    dec = dict(d_sep=4.0, margin=1.0, d_look=30.0)
    rows = np.zeros((4, d2dhip.SCEN_STRIDE))
    rows[:, d2dhip.SC_VMAX] = 14.0
    W0 = np.zeros((4, 5, 6))
    with pytest.raises(NotImplementedError, match='polynomial fit has no deconfliction'):
        full_sim.plan_batch(rows, 50, 4.9, 0.1, deconflict=dec)
    for name, kw in (('free_time', dict(free_time=(0.05, 0.2))), ('keep_out', dict(keep_out=np.zeros((4, 1, 3)))), ('via', dict(via=[[]] * 4))):
        with pytest.raises(NotImplementedError, match=f'deconflict with {name}'):
            full_sim.plan_batch(rows, 6, 0.5, 0.1, backend='nlp', W0=W0, h=0.1, deconflict=dec, **kw)
    with pytest.raises(ValueError, match='missing'):
        full_sim.plan_batch(rows, 6, 0.5, 0.1, backend='nlp', W0=W0, h=0.1, deconflict=dict(d_sep=4.0))
    with pytest.raises(ValueError, match='off the common row grid'):
        full_sim.plan_batch(rows, 6, 0.5, 0.1, backend='nlp', W0=W0, h=0.1, n_ac=2, t_start=torch.tensor([0.0, 0.25], dtype=torch.float64), deconflict=dec)
    # deconflict=None: the solve and nothing else; with a dict: the loop after it, on the clock of t_start
    ctx = _Stub([([0, 0], [[-1] * 8] * 2)], 2, 8)
    monkeypatch.setattr(d2dhip, 'default_context', lambda: ctx)
    out = full_sim.plan_batch(rows, 6, 0.5, 0.1, backend='nlp', W0=W0, h=0.1, n_ac=2)
    assert [c[0] for c in ctx.calls] == ['nlp_solve_groups'] and 'deconflict' not in out
    ctx.calls.clear()
    out = full_sim.plan_batch(rows, 6, 0.5, 0.1, backend='nlp', W0=W0, h=0.1, n_ac=2, t_start=torch.tensor([1.3, 1.0], dtype=torch.float64), deconflict=dec)
    assert [c[0] for c in ctx.calls] == ['nlp_solve_groups', 'fleet_tracks', 'fleet_audit'] and out['deconflict']['rounds'] == 0
    assert ctx.calls[1][1]['row0'].tolist() == [3, 0] and ctx.calls[1][1]['t0'] == 1.0
