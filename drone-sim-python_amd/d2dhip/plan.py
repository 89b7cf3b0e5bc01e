"""Which collocation entry a planner calls: policy above the binding, no ctypes (d2dhip.nlp_plan).  The rule is the two tables."""

WIND = ('field', 't_start')
MOVING = ('knots', 'disc') + WIND
HARD = ('hard_knots', 'hard_disc') + WIND

# The sixteen entries nlp_plan can choose, in precedence order: (entry, a group launch (n_ac given: R scenarios of n_ac aircraft) or the
# hand-out of B problems (n_ac None), the input that names it, the inputs handed by position behind h, the inputs handed by keyword).
# The first row of the call's launch shape whose naming input is given is the entry; a group entry takes n_ac by keyword unless by position.
ENTRIES = (
    ('nlp_solve_free_fence', False, 'window', ('window',), ('keep', 'fence')),   # the step free beside static hard discs and a geofence
    ('nlp_solve_groups_fence', True, 'fence', ('n_ac', 'fence'), WIND),          # one polygon per scenario [R][n_edge][4]; no hard discs
    ('nlp_solve_fence', False, 'fence', ('fence',), ('keep',) + WIND),           # GeoFence.lowered() [B][n_edge][4], static hard discs beside it
    ('nlp_solve_groups_keepout', True, 'hard_knots', (), HARD),                  # HARD discs that move: nlp_solve_moving's tables, disc[.., 0]
    ('nlp_solve_keepout_moving', False, 'hard_knots', (), HARD),                 # the node radius
    ('nlp_solve_keepout', False, 'keep', ('keep',), WIND),                       # static hard discs [B][n_keep][3]
    ('nlp_solve_groups_via', True, 'via', (), ('via',) + MOVING),
    ('nlp_solve_groups_moving', True, 'knots', (), MOVING),
    ('nlp_solve_groups_pairs', True, 'pairs', (), WIND),
    ('nlp_solve_groups_wind', True, 'field', (), WIND),
    ('nlp_solve_groups', True, None, (), ()),
    ('nlp_solve_free', False, 'free_rows', (), ('free_rows',)),
    ('nlp_solve_via', False, 'via', (), ('via',) + MOVING),
    ('nlp_solve_moving', False, 'knots', (), MOVING),
    ('nlp_solve_wind', False, 'field', (), WIND),
    ('nlp_solve', False, None, (), ()),
)
# the entries' own keyword of an input that they spell differently
KEYWORD = dict(keep='discs', fence='edges', hard_knots='knots', hard_disc='disc')

# The leading input (the first of these that is given) -> the inputs it refuses (the first one given is the one named) and why.
REFUSES = {
    'window': (('n_ac', 'field', 'via', 'knots', 'disc', 'hard_knots', 'hard_disc', 'free_rows'),
               'a free step holds static hard discs and a geofence for one aircraft in the rows\' constant wind, without pins or anything '
               'that moves (window replaces free_rows)'),
    'fence': (('free_rows', 'via', 'knots', 'disc', 'hard_knots', 'hard_disc'),
              'a geofence goes with static hard discs (one aircraft) and a fixed step, not with moving discs, pins or a free step'),
    'hard_knots': (('keep', 'knots', 'disc', 'via', 'free_rows'),
                   'hard moving discs go with neither static hard discs, soft moving discs, pins nor a free step'),
    'keep': (('n_ac', 'free_rows', 'via', 'knots'), 'hard keep-out discs are for one aircraft on static discs with a fixed step'),
}


def nlp_plan(ctx, scen, W, h, *, n_ac=None, field=None, t_start=None, knots=None, disc=None, via=None, free_rows=None, pairs=False, keep=None,
             hard_knots=None, hard_disc=None, fence=None, window=None, **opts):
    """The planners' one rule for choosing among the nlp_solve* methods of `ctx` (a Context, or any object that has them): REFUSES says
    which inputs do not combine -- each pair is refused by name -- and ENTRIES which entry the inputs that are given name and what it
    is handed; an input that the entry does not take is not looked at (free_rows: everything but itself).  free_rows keeps refusing
    keep and fence through theirs: window is the spelling of a free step beside them, its rows those of free_rows.
    opts: the entry's own keywords (solver options, bounds, max_sweeps ...).  Returns the entry's dictionary plus `entry`, its name.
    (nlp_solve_model is not chosen here: its objective model is another problem, not an optional input of a plan -- DESIGN.md 5.16.)"""
    inp = dict(n_ac=n_ac, field=field, t_start=t_start, knots=knots, disc=disc, via=via, free_rows=free_rows, pairs=pairs or None, keep=keep,
               hard_knots=hard_knots, hard_disc=hard_disc, fence=fence, window=window)
    given = {k for k, v in inp.items() if v is not None}
    if 'hard_disc' in given:                     # either table of the hard moving discs leads, under the name of the first
        given.add('hard_knots')
    lead = next((k for k in REFUSES if k in given), None)
    if lead is not None:
        names, why = REFUSES[lead]
        for name in names:
            if inp[name] is not None:
                raise NotImplementedError(f'{lead} together with {name}: {why}')
    if lead == 'fence' and n_ac is not None and keep is not None:        # (a triple, so not a row of REFUSES)
        raise NotImplementedError('fence together with keep and n_ac: the group entry carries no hard discs; plan one aircraft at a '
                                  'time (nlp_solve_fence)')
    if lead == 'hard_knots' and (hard_knots is None or hard_disc is None):
        raise ValueError('hard_knots and hard_disc go together')
    entry, groups, _, pos, takes = next(row for row in ENTRIES if row[1] == (n_ac is not None) and (row[2] is None or row[2] in given))
    kw = {KEYWORD.get(k, k): inp[k] for k in takes}
    if groups and 'n_ac' not in pos:
        kw['n_ac'] = n_ac
    if entry == 'nlp_solve_wind' and t_start is None:          # (its t_start is a float with a default; every other entry takes None)
        kw['t_start'] = 0.0
    out = getattr(ctx, entry)(scen, W, h, *(inp[k] for k in pos), **kw, **opts)
    out['entry'] = entry
    return out
