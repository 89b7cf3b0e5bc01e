"""Which collocation entry a planner calls: policy above the binding, no ctypes (d2dhip.nlp_plan)."""


def nlp_plan(ctx, scen, W, h, *, n_ac=None, field=None, t_start=None, knots=None, disc=None, via=None, free_rows=None, pairs=False, keep=None,
             hard_knots=None, hard_disc=None, fence=None, window=None, **opts):
    """The planners' one rule for choosing among the nlp_solve* methods of `ctx` (a Context, or any object that has them) -- the first
    optional input that is given names the entry, which also takes the inputs below it in its column (free_rows: none):
      n_ac given, R scenarios of n_ac aircraft:  via -> _groups_via, knots -> _groups_moving, pairs -> _groups_pairs, field -> _groups_wind,
                                                 none -> nlp_solve_groups;
      n_ac None, B problems handed out:          free_rows -> _free, via -> _via, knots -> _moving, field -> _wind, none -> nlp_solve.
    keep given (n_ac None, no free_rows, via or knots -- each pair refused by name): nlp_solve_keepout with field and t_start.
    hard_knots / hard_disc given (HARD discs that move: the tables of nlp_solve_moving with disc[.., 0] the node radius): n_ac None ->
    nlp_solve_keepout_moving, n_ac given -> nlp_solve_groups_keepout, with field and t_start; refused by name together with keep, knots /
    disc, via or free_rows.
    fence given (the rows of d2d.opty_utils.GeoFence.lowered()): n_ac None -> nlp_solve_fence (dev [B][n_edge][4]) with keep (its static
    hard discs), n_ac given -> nlp_solve_groups_fence (dev [R][n_edge][4], one polygon per scenario; keep refused by name), with field and
    t_start; refused by name together with free_rows, via, knots / disc or hard_knots / hard_disc.
    window given (the rows of free_rows, dev [B][4] = (h_lo, h_hi, k_dur, h_start): the leg's duration free WHILE static hard discs and
    a geofence are held): nlp_solve_free_fence with keep and fence (either or both may be None); refused by name together with n_ac,
    field, via, knots / disc, hard_knots / hard_disc or free_rows.  (free_rows keeps refusing keep and fence: window is the spelling.)
    opts: the entry's own keywords (solver options, bounds, max_sweeps ...).  Returns the entry's dictionary plus `entry`, its name.
    (nlp_solve_model is not chosen here: its objective model is another problem, not an optional input of a plan -- DESIGN.md 5.16.)"""
    wind = dict(field=field, t_start=t_start)
    if window is not None:
        for name, given in (('n_ac', n_ac is not None), ('field', field is not None), ('via', via is not None), ('knots', knots is not None),
                            ('disc', disc is not None), ('hard_knots', hard_knots is not None), ('hard_disc', hard_disc is not None),
                            ('free_rows', free_rows is not None)):
            if given:
                raise NotImplementedError(f'window together with {name}: a free step holds static hard discs and a geofence for one aircraft '
                                          'in the rows\' constant wind, without pins or anything that moves (window replaces free_rows)')
        out = ctx.nlp_solve_free_fence(scen, W, h, window, discs=keep, edges=fence, **opts)
        out['entry'] = 'nlp_solve_free_fence'
        return out
    if fence is not None:
        for name, given in (('free_rows', free_rows is not None), ('via', via is not None), ('knots', knots is not None),
                            ('disc', disc is not None), ('hard_knots', hard_knots is not None), ('hard_disc', hard_disc is not None)):
            if given:
                raise NotImplementedError(f'fence together with {name}: a geofence goes with static hard discs (one aircraft) and a fixed step, '
                                          'not with moving discs, pins or a free step')
        if n_ac is not None:
            if keep is not None:
                raise NotImplementedError('fence together with keep and n_ac: the group entry carries no hard discs; plan one aircraft at a '
                                          'time (nlp_solve_fence)')
            out = ctx.nlp_solve_groups_fence(scen, W, h, n_ac, fence, **wind, **opts)
            out['entry'] = 'nlp_solve_groups_fence'
            return out
        out = ctx.nlp_solve_fence(scen, W, h, fence, discs=keep, **wind, **opts)
        out['entry'] = 'nlp_solve_fence'
        return out
    if hard_knots is not None or hard_disc is not None:
        for name, given in (('keep', keep is not None), ('knots', knots is not None), ('disc', disc is not None), ('via', via is not None),
                            ('free_rows', free_rows is not None)):
            if given:
                raise NotImplementedError(f'hard_knots together with {name}: hard moving discs go with neither static hard discs, soft moving '
                                          'discs, pins nor a free step')
        if hard_knots is None or hard_disc is None:
            raise ValueError('hard_knots and hard_disc go together')
        entry = 'nlp_solve_keepout_moving' if n_ac is None else 'nlp_solve_groups_keepout'
        kw = dict(knots=hard_knots, disc=hard_disc, **wind)
        if n_ac is not None:
            kw['n_ac'] = n_ac
        out = getattr(ctx, entry)(scen, W, h, **kw, **opts)
        out['entry'] = entry
        return out
    if keep is not None:
        # hard keep-out discs (dev [B][n_keep][3]): nlp_solve_keepout, with the field and the start times; alone among the optional inputs
        for name, given in (('n_ac', n_ac is not None), ('free_rows', free_rows is not None), ('via', via is not None), ('knots', knots is not None)):
            if given:
                raise NotImplementedError(f'keep together with {name}: hard keep-out discs are for one aircraft on static discs with a fixed step')
        out = ctx.nlp_solve_keepout(scen, W, h, keep, **wind, **opts)
        out['entry'] = 'nlp_solve_keepout'
        return out
    mov = dict(knots=knots, disc=disc, **wind)
    if n_ac is not None:
        entry, kw = (('nlp_solve_groups_via', dict(via=via, **mov)) if via is not None else
                     ('nlp_solve_groups_moving', mov) if knots is not None else
                     ('nlp_solve_groups_pairs', wind) if pairs else
                     ('nlp_solve_groups_wind', wind) if field is not None else ('nlp_solve_groups', {}))
        kw['n_ac'] = n_ac
    else:
        entry, kw = (('nlp_solve_free', dict(free_rows=free_rows)) if free_rows is not None else
                     ('nlp_solve_via', dict(via=via, **mov)) if via is not None else
                     ('nlp_solve_moving', mov) if knots is not None else
                     ('nlp_solve_wind', dict(field=field, t_start=0.0 if t_start is None else t_start)) if field is not None else ('nlp_solve', {}))
    out = getattr(ctx, entry)(scen, W, h, **kw, **opts)
    out['entry'] = entry
    return out
