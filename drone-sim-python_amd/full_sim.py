"""Script-level simulation functions of src/11_full_sim_case1.py (that file runs main() at
import, so its functions are mirrored here under their own names) with the time loops on the
GPU, plus batched variants over many independent formations.

  CircularFormationGVF(c, r, v, n_ac, X0f, ...)      src/11_full_sim_case1.py:93-177
  implement_controller(n_ac, time, x_ref, y_ref, ..)  :241-291
  ConstructBMatrix, ComputeDerivatives, ExtractTrajData, ExtendTraj_symm   :81-91, :197-239
  run_simulation(time, aircraft, windfield, ctl, X0, perts)                src/05_test_simulation.py:21-34 (legacy DFFF loop)

Wind: the constant WindField classes take the constant-wind loops as before; a d2d.wind.SplineWindField (windfield=) is flown by
the plant at each aircraft's own position and time (the reference's WindField.sample plug-point); any other field with its own
sample() raises NotImplementedError (d2d.wind.plant_wind) instead of being frozen at one sample.
Gusts: gust= (a d2d.wind.GustModel) adds a stochastic gust per aircraft, drawn inside the device loops, to whichever wind the plant
flies; the controllers never see it.  The planners take none: a gust is a property of the plant, not of a plan.
"""
import numpy as np

import d2dhip
import d2d.dynamic as ddyn
import d2d.multiopty_utils as d2mou
from d2d.wind import plant_gust, plant_wind, wind_estimator

KE, KD, KR = 0.0004, 25, 20            # src/11_full_sim_case1.py:108-110
X1_START = np.array([20, 30, -np.pi / 2, 0, 10])     # :113


def ConstructBMatrix(n_ac):
    B = np.zeros((n_ac, n_ac - 1))
    for j in range(n_ac - 1):
        B[j, j], B[j + 1, j] = -1, 1
    return B


def _planes(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)


def hold_steps(t_opt_comp, t_step):
    """How many further steps the phase-error rule must hold before the reference's case-3 loop breaks: it adds t_step to a
    running dt on every such step and breaks once dt >= t_opt_comp (src/12_full_sim_case3.py:163-178); same floating-point sum."""
    k, acc = 0, 0.0
    while not acc >= t_opt_comp:
        acc += t_step
        k += 1
    return k


def _audit_kw(ctx, audit, n_form, what):
    """The flight_audit arguments of an `audit=` value: True, or a dict of d_safe (m; rows closer than it are counted), err_tol (m) and
    static (discs (n_stat, 3) = (x, y, r) for every formation, or (n_form, n_stat, 3)); `what`: further keys this caller accepts."""
    audit = {} if audit is True else dict(audit)
    unknown = set(audit) - {'d_safe', 'err_tol', 'static'} - set(what)
    if unknown:
        raise ValueError(f'audit: unknown keys {sorted(unknown)}')
    kw = dict(d_safe=float(audit.get('d_safe', 0.0)), err_tol=float(audit.get('err_tol', np.inf)))
    if audit.get('static') is not None:
        st = np.asarray(audit['static'], dtype=np.float64)
        kw['static'] = ctx.dev(np.ascontiguousarray(np.broadcast_to(st, (n_form,) + st.shape[-2:])))
    return kw


def fleet_row0(t_start, dt_row):
    """The global rows of formations that start at t_start [n_form] on a history of row spacing dt_row: (t_start - min t_start) /
    dt_row as int32.  The fleet audit compares formations on integer rows: a formation more than 1e-9 rows off the common grid is
    refused by name (host only)."""
    t = np.asarray(t_start, dtype=np.float64).reshape(-1)
    u = (t - t.min()) / float(dt_row)
    r = np.rint(u)
    bad = np.nonzero(~(np.abs(u - r) <= 1e-9))[0]
    if bad.size:
        f = int(bad[0])
        raise ValueError(f'fleet audit: formation {f} starts {float(u[f])!r} rows after the earliest formation, off the common row grid '
                         f'(dt_row = {float(dt_row)!r}): the cross-formation audit compares formations on whole rows')
    return r.astype(np.int32)


def _fleet_audit(ctx, audit, X, n_ac, dt_row, n_form, rows=None, t_start=None, layout='hist'):
    """Context.fleet_audit of a history for the `fleet=` entry of an `audit=` value (None when there is none): a dict of d_look and
    step_max (m, required), world ((n_form,) integers, optional), d_safe, tile_rows, slots.  t_start: None or a float (one clock) or
    a device tensor [n_form] of the formations' own start times, which fleet_row0 turns into rows (read on the host)."""
    fleet = None if audit is True or audit is None else audit.get('fleet')
    if fleet is None:
        return None
    fleet = dict(fleet)
    unknown = set(fleet) - {'d_look', 'step_max', 'world', 'd_safe', 'tile_rows', 'slots'}
    if unknown or 'd_look' not in fleet or 'step_max' not in fleet:
        raise ValueError(f'audit: fleet needs d_look and step_max and takes world, d_safe, tile_rows, slots (unknown: {sorted(unknown)})')
    kw = {k: fleet[k] for k in ('d_safe', 'tile_rows', 'slots') if k in fleet}
    if fleet.get('world') is not None:
        kw['world'] = ctx.dev(np.array(np.broadcast_to(np.asarray(fleet['world'], dtype=np.int32), (n_form,))))
    if t_start is not None and np.ndim(t_start) > 0:
        ts = t_start.cpu().numpy() if hasattr(t_start, 'cpu') else np.asarray(t_start)
        kw['row0'] = ctx.dev(fleet_row0(ts, dt_row))
    return ctx.fleet_audit(X, n_ac, dt_row, float(fleet['d_look']), float(fleet['step_max']), rows=rows, layout=layout, **kw)


def CircularFormationGVF_batch(c, r, v, n_ac, X0f=None, t_start=0, t_step=0.05, t_end=1000, X0=None,
                               tau_phi=None, rec_stride=1, record=('X', 'U', 'Rr', 'eth'), W=(0., 0.), etheta_tol_deg=None,
                               t_opt_comp=0.0, windfield=None, audit=None, gust=None, gust_state=None, gust_phase=0, gust_stream_base=0,
                               wind_estimate=None):
    """Many formations at once.  c (n_form, n_ac, 2) centres; r scalar or (n_form, n_ac); X0
    (n_form, n_ac, 5) or None (every aircraft starts at the reference's X1); X0f (n_form, n_ac, >=3)
    or None.  etheta_tol_deg: stop by the phase-error rule of cases 2 / 3 instead of the state rule (after t_opt_comp more seconds on
    which it holds).  windfield: a SplineWindField the plant flies instead of W (row i at t_start + i t_step; the GVF law never reads
    the wind).  Returns the raw device dictionary of d2dhip.Context.gvf_run plus `time`.
    audit: True or a dict (d_safe, err_tol, static: _audit_kw) -- out['audit'] is Context.flight_audit of the recorded history: every
    formation's rows up to its stop row (derived on the device), dt_row = t_step rec_stride; needs 'X' in record.  With
    fleet=dict(d_look=, step_max=, world=...) in the dict, out['audit']['fleet'] is Context.fleet_audit of the same rows: the
    separation between aircraft of different formations (_fleet_audit; times from the first row).
    gust: a d2d.wind.GustModel flown on top of W or the field (the law sees none of it); gust_state dev [4][N] or None (the stationary
    start), gust_phase: the loop's phase word, gust_stream_base: the global index of the first drone (a shard of a larger batch).
    out['gust_state'] dev [4][N]: the state after each formation's last executed step; with 'g' in record out['g'] dev [n_rec][2][N].
    wind_estimate: a d2d.wind.WindEstimator -- out['wind_estimate'] is the WindEstimate fitted to the flight just made (d2d_wind_fit on
    the recorded history: every formation's rows up to its stop row, dt_row = t_step rec_stride); needs 'X' in record."""
    if audit is not None and 'X' not in record:
        raise ValueError("audit needs the state history: 'X' must be in record")
    est = wind_estimator(wind_estimate)
    if est is not None and 'X' not in record:
        raise ValueError("wind_estimate needs the state history: 'X' must be in record")
    fld = plant_wind(windfield)
    gkw = {} if plant_gust(gust) is None else dict(gust=gust, gust_state=gust_state, gust_phase=gust_phase, gust_stream_base=gust_stream_base)
    ctx = d2dhip.default_context()
    c = np.asarray(c, dtype=np.float64).reshape(-1, n_ac, 2)
    n_form = c.shape[0]
    N = n_form * n_ac
    time = np.arange(t_start, t_end, t_step)
    X0 = np.tile(X1_START, (N, 1)) if X0 is None else np.asarray(X0, dtype=np.float64).reshape(N, 5)
    R = np.broadcast_to(np.asarray(r, dtype=np.float64), (n_form, n_ac)).reshape(N) if np.ndim(r) else np.full(N, float(r))
    ac = ddyn.Aircraft()
    x0f = None if X0f is None else ctx.dev(_planes(np.asarray(X0f, dtype=np.float64).reshape(N, -1)[:, :3]))
    out = ctx.gvf_run(ctx.dev(_planes(X0)), ctx.dev(_planes(c.reshape(N, 2))), ctx.dev(np.ascontiguousarray(R)), n_ac,
                      len(time), t_step, float(v), KE, KD, KR, B=ConstructBMatrix(n_ac), z_des=np.zeros(max(n_ac - 1, 0)),
                      tau_phi=ac.tau_phi if tau_phi is None else tau_phi, tau_v=ac.tau_v, W=W, X0f=x0f,
                      rec_stride=rec_stride, record=record, etheta_tol_deg=etheta_tol_deg,
                      stop_hold=hold_steps(t_opt_comp, t_step) if etheta_tol_deg is not None else 0,
                      **({} if fld is None else dict(wind=fld, t_start=float(time[0]))), **gkw)
    out['time'] = time
    if audit is not None or est is not None:
        torch = d2dhip._torch()
        rows = ((torch.clamp(out['stop_row'], max=len(time)) + (rec_stride - 1)) // rec_stride).to(torch.int32)
    if audit is not None:
        kw = _audit_kw(ctx, audit, n_form, ('fleet',))
        out['audit'] = ctx.flight_audit(out['X'], n_ac, t_step * rec_stride, rows=rows, t_start=float(time[0]), **kw)
        fleet = _fleet_audit(ctx, audit, out['X'], n_ac, t_step * rec_stride, n_form, rows=rows)
        if fleet is not None:
            out['audit']['fleet'] = fleet
    if est is not None:
        out['wind_estimate'] = est.fit(ctx, out['X'], n_ac, t_step * rec_stride, rows=rows, t_start=float(time[0]))
    return out


def CircularFormationGVF(c, r, v, n_ac, X0f, t_start=0, t_step=0.05, t_end=1000):
    """One formation, the reference's 8-tuple: X_array, U_array, U1_array, U2_array, Ur_array,
    e_theta_array, time, t_f -- trimmed at the stop row like the reference (its U2 slice quirk,
    `U2_array[i,:]`, is reproduced)."""
    out = CircularFormationGVF_batch(np.asarray(c)[None], r, v, n_ac, X0f=np.asarray(X0f, dtype=float)[None],
                                     t_start=t_start, t_step=t_step, t_end=t_end)
    d2dhip.default_context().sync()
    time = out['time']
    i = int(out['stop_row'].cpu().numpy()[0])
    X = out['X'].cpu().numpy().transpose(0, 2, 1)
    U = out['U'].cpu().numpy().transpose(0, 2, 1)
    Rr = out['Rr'].cpu().numpy(); eth = out['eth'].cpu().numpy()
    # U1/U2 (debug decomposition of the GVF command) are not kept by the fused loop
    U1 = np.zeros((len(time), n_ac)); U2 = np.zeros((len(time), n_ac))
    if i < len(time):
        t_f = time[i - 1]
        return X[:i], U[:i], U1[:i], U2[i, :], Rr[:i], eth[:i], time[:i], t_f
    return X, U, U1, U2, Rr, eth, time, t_end


def _gvf_trimmed(out, n_ac, t_end):
    d2dhip.default_context().sync()
    time = out['time']
    rows = int(out['stop_row'].cpu().numpy()[0])
    X = out['X'].cpu().numpy().transpose(0, 2, 1); U = out['U'].cpu().numpy().transpose(0, 2, 1)
    Rr = out['Rr'].cpu().numpy(); eth = out['eth'].cpu().numpy()
    U1 = np.zeros((len(time), n_ac)); U2 = np.zeros((len(time), n_ac))        # (debug decomposition, not kept by the fused loop)
    fired = rows < len(time) or bool(out['conv_row'].cpu().numpy()[0] >= 0 and rows == len(time))
    return X, U, U1, U2, Rr, eth, time, rows, fired


def CircularFormationGVF_case2(c, r, v, n_ac, t_start=0, t_step=0.05, t_end=1000, etheta_tol=0.5):
    """src/12_full_sim_case2.py:85-164: the circular-formation phase that ends when every inter-vehicle phase error is <= 0.5 deg.
    The reference's 8-tuple, trimmed to [:i+1] (its `U2_array[i+1,:]` slice quirk reproduced), t_f = time[i-1]."""
    out = CircularFormationGVF_batch(np.asarray(c)[None], r, v, n_ac, t_start=t_start, t_step=t_step, t_end=t_end,
                                     etheta_tol_deg=etheta_tol)
    X, U, U1, U2, Rr, eth, time, rows, fired = _gvf_trimmed(out, n_ac, t_end)
    if fired and rows < len(time):
        return X[:rows], U[:rows], U1[:rows], U2[rows, :], Rr[:rows], eth[:rows], time[:rows], time[rows - 2]
    return X, U, U1, U2, Rr, eth, time, t_end


def CircularFormationGVF_case3(c, r, v, n_ac, t_start=0, t_step=0.05, t_end=1000, etheta_tol=2., t_opt_comp=0.7):
    """src/12_full_sim_case3.py:85-181: as case 2 with a 2 deg tolerance, flying on for t_opt_comp seconds after the first
    convergence (the time the planner takes); the last element is the reference's convergence = [index, t_convergence, t_f]."""
    out = CircularFormationGVF_batch(np.asarray(c)[None], r, v, n_ac, t_start=t_start, t_step=t_step, t_end=t_end,
                                     etheta_tol_deg=etheta_tol, t_opt_comp=t_opt_comp)
    X, U, U1, U2, Rr, eth, time, rows, fired = _gvf_trimmed(out, n_ac, t_end)
    idx = int(out['conv_row'].cpu().numpy()[0])
    if rows < len(time):
        conv = [idx, time[idx], time[rows - 2]]
        return X[:rows], U[:rows], U1[:rows], U2[rows, :], Rr[:rows], eth[:rows], time[:rows], conv
    return X, U, U1, U2, Rr, eth, time, [idx, time[idx] if idx >= 0 else None, None]


def trajectory_gen_multi(p, delta):
    """A second aircraft flying the single-aircraft plan shifted by delta (src/12_full_sim_case3.py:195-201): sol_x, sol_y (N, 2)."""
    x, y = p.sol_x.reshape(-1, 1), p.sol_y.reshape(-1, 1)
    p.sol_x, p.sol_y = np.append(x, x + delta[0], axis=1), np.append(y, y + delta[1], axis=1)
    return p


def trajectory_optimization_single(scen, delta, backend=None):
    """src/12_full_sim_case3.py:184-193 without the plots: one single-aircraft plan (scen.p0 injected by the caller, :456-460),
    duplicated with an offset for the wingman.  A scenario with t1_free is planned with its duration free (single_opt_planner): both
    aircraft then share the solved clock p.sol_time, p.time_step, p.duration."""
    import single_opt_planner as sop
    p = sop.Planner(scen, backend=backend)
    p.configure(tol=1e-5, max_iter=1500)
    p.run(initial_guess=p.get_initial_guess())
    return trajectory_gen_multi(p, delta)


def ComputeDerivatives(x_ref, y_ref, dt):
    """Two passes of second-order-edge central differences (src/11_full_sim_case1.py:197-204); the
    tracking kernel computes the same on the device -- this host version serves callers that only
    want the derivatives."""
    Fdx = np.gradient(x_ref, edge_order=2) / dt
    Fdy = np.gradient(y_ref, edge_order=2) / dt
    return Fdx, Fdy, np.gradient(Fdx, edge_order=2) / dt, np.gradient(Fdy, edge_order=2) / dt


def ExtractTrajData(df, n_ac):
    """CSV columns time, x_i, y_i, psi_i (1-based) -> arrays (src/11_full_sim_case1.py:206-217)."""
    t = np.array(df['time'])
    cols = lambda k: np.stack([np.array(df[f'{k}_{i + 1}']) for i in range(n_ac)], 1)   # noqa: E731
    return t, cols('x'), cols('y'), cols('psi')


def ExtendTraj_symm(n_ac, x_ref, y_ref, psi_ref, time):
    """Append the mirrored half taken from the aircraft whose start equals this one's end
    (src/11_full_sim_case1.py:219-239; psi is extended with y values, as the reference does)."""
    time = np.append(time, time + time[-1])
    x0, xf, y0, yf = x_ref[0, :], x_ref[-1, :], y_ref[0, :], y_ref[-1, :]
    ax = [int(np.nonzero((x0 == xf[i]) & (y0 == yf[i]))[0][0]) for i in range(n_ac)]
    xs, ys = x_ref[:, ax], y_ref[:, ax]
    return time, np.append(x_ref, xs, axis=0), np.append(y_ref, ys, axis=0), np.append(psi_ref, ys, axis=0)


def implement_controller_batch(time, x_ref, y_ref, w, X0s, record=('X', 'U', 'Xr', 'dX', 'Yd', 'Ydd'), windfield=None, audit=None,
                               gust=None, gust_state=None, gust_phase=0, gust_n_ac=1, gust_stream_base=0, wind_estimate=None):
    """x_ref, y_ref (T, n) for n independent drones; X0s (n, 5).  Device dictionary out.  windfield: a SplineWindField the plant
    flies (row i at time[i]); the controller keeps w, as DiffController(w) does (src/11_full_sim_case1.py:241-291).
    audit: True or a dict (d_safe, err_tol, static: _audit_kw; n_ac: consecutive drones that form a formation, default 1 -- the
    drones are independent) -- out['audit'] is Context.flight_audit of the flown history against x_ref, y_ref; needs 'X' in record.
    With fleet=dict(d_look=, step_max=, ...) in the dict, out['audit']['fleet'] is Context.fleet_audit of the same history.
    gust: a d2d.wind.GustModel flown on top of w or the field (the controller sees none of it); gust_state, gust_phase,
    gust_stream_base as in CircularFormationGVF_batch, gust_n_ac: consecutive drones that share the formation part of the gust.
    out['gust_state'] dev [4][n]; with 'g' in record out['g'] dev [T][2][n].
    wind_estimate: a d2d.wind.WindEstimator -- out['wind_estimate'] is the WindEstimate fitted to the flown history (every drone its
    own formation, row i at time[i]); needs 'X' in record."""
    if audit is not None and 'X' not in record:
        raise ValueError("audit needs the state history: 'X' must be in record")
    est = wind_estimator(wind_estimate)
    if est is not None and 'X' not in record:
        raise ValueError("wind_estimate needs the state history: 'X' must be in record")
    fld = plant_wind(windfield)
    gkw = {} if plant_gust(gust) is None else dict(gust=gust, gust_state=gust_state, gust_phase=gust_phase, gust_n_ac=gust_n_ac,
                                                   gust_stream_base=gust_stream_base)
    ctx = d2dhip.default_context()
    ac = ddyn.Aircraft()
    dt = time[1] - time[0]
    xr, yr = ctx.dev(np.ascontiguousarray(x_ref, dtype=np.float64)), ctx.dev(np.ascontiguousarray(y_ref, dtype=np.float64))
    out = ctx.track_run(xr, yr, ctx.dev(_planes(np.asarray(X0s, dtype=np.float64))), float(dt), record=record,
                        w=(float(w[0]), float(w[1])), **_track_constants(ac),
                        **({} if fld is None else dict(wind=fld, t_start=float(time[0]))), **gkw)
    if audit is not None:
        n_ac = 1 if audit is True else int(audit.get('n_ac', 1))
        kw = _audit_kw(ctx, audit, xr.shape[1] // n_ac, ('n_ac', 'fleet'))
        out['audit'] = ctx.flight_audit(out['X'], n_ac, float(dt), t_start=float(time[0]), x_ref=xr, y_ref=yr, **kw)
        fleet = _fleet_audit(ctx, audit, out['X'], n_ac, float(dt), xr.shape[1] // n_ac)
        if fleet is not None:
            out['audit']['fleet'] = fleet
    if est is not None:
        out['wind_estimate'] = est.fit(ctx, out['X'], 1, float(dt), t_start=float(time[0]))
    return out


def _track_constants(ac=None):
    """The controller constants of the tracking loop that are not Context.track_params' defaults (Q, R, the saturations): the lags of
    d2d.dynamic.Aircraft.  implement_controller_batch and track_dispersion both take them from here."""
    ac = ddyn.Aircraft() if ac is None else ac
    return dict(tau_phi=ac.tau_phi, tau_v=ac.tau_v)


def track_dispersion(time, x_ref, y_ref, w, gust, fence=None, keep_out=None, S0=None, record_P=False, windfield=None, loop='track'):
    """The gust dispersion of implement_controller_batch(time, x_ref, y_ref, w, X0s, gust=gust): how far the LQR-tracked flight
    strays from its gust-free self, as a covariance per row, from ONE deterministic pass per plan (Context.track_dispersion,
    include/d2d.h d2d_track_dispersion) instead of thousands of flown replicas.  x_ref, y_ref (T, n) for n independent drones, w the
    constant wind, gust a d2d.wind.GustModel; fence: a d2d.opty_utils.GeoFence or lowered rows, keep_out: discs (k, 3) = (cx, cy, R);
    S0 dev [28][n] to continue an earlier report's 'S'; record_P: keep 'Ppos' dev [T][3][n].  The controller constants are
    implement_controller_batch's own (_track_constants and Context.track_params' defaults).
    Returns Context.track_dispersion's dict of device tensors plus 'gust', the model; dispersion_margin turns it into margins.
    The saturations (err_sats, phi_lim, v_min / v_max) and the heading wrap are not modelled.  Refused: a SplineWindField (its
    gradient would enter the plant's Jacobian), the GVF formation loop and the legacy dfff_run loop (loop='gvf' / 'dfff')."""
    if loop == 'gvf':
        raise NotImplementedError('track_dispersion covers the LQR tracking loop only: the GVF formation loop (CircularFormationGVF_batch) '
                                  'is a nonlinear guidance law with a coupled formation controller')
    if loop == 'dfff':
        raise NotImplementedError('track_dispersion covers the LQR tracking loop only: the legacy dfff_run loop (run_simulation_batch) has '
                                  'another gain and another reference pairing')
    if loop != 'track':
        raise ValueError(f"loop={loop!r}: 'track' (or 'gvf', 'dfff', both refused)")
    if windfield is not None:
        raise NotImplementedError(f'track_dispersion in a {type(windfield).__name__}: the gradient of a SplineWindField would enter the '
                                  "plant's Jacobian; only the constant wind w is covered")
    if plant_gust(gust) is None:
        raise TypeError('NoneType is not a gust model: build one with d2d.wind.GustModel(sigma, tau=...)')
    ctx = d2dhip.default_context()
    xr, yr = ctx.dev(np.ascontiguousarray(x_ref, dtype=np.float64)), ctx.dev(np.ascontiguousarray(y_ref, dtype=np.float64))
    out = ctx.track_dispersion(xr, yr, w=(float(w[0]), float(w[1])), gust=gust, dt=float(time[1] - time[0]), fence=fence, keep_out=keep_out,
                               S0=S0, record_P=record_P, **_track_constants())
    out['gust'] = gust
    return out


def dispersion_margin(report, prob, pair=None):
    """Margins from a track_dispersion report: z_prob times the predicted standard deviation, z_prob the one-sided normal quantile of
    `prob` (1.35e-3 -> 3.0).  Returns dict(z, disc [n]: z sig_max, what KeepOut(margin=) of any disc may take; fence [k][n]:
    z fence_sn per edge, what GeoFence(margin=) may take (with a fence in the report); pair: with pair=(i, j) the same for the
    distance between drones i and j, z sqrt(sig_max_i^2 + sig_max_j^2), for deconflict(d_sep=)).
    What the figure is: `prob` is the chance that the GUST SHARE of the deviation, along one constraint's normal, exceeds the margin
    at ONE row -- per row and per constraint.  It is NOT a probability over the whole flight (a flight has many rows and their
    deviations are correlated; the chance of one exceedance somewhere is larger), and it does NOT contain the gust-free tracking
    error, which flight_audit reports as err_max and the caller adds.
    pair needs form_corr = 0: with a shared gust part the two aircraft's deviations are correlated and their cross-covariance is
    not computed (refused); with form_corr = 0 the relative covariance is P_i + P_j, bounded here by the two largest eigenvalues."""
    from statistics import NormalDist
    if not (np.isfinite(prob) and 0.0 < prob < 0.5):
        raise ValueError(f'prob={prob!r} must be in (0, 0.5): a one-sided exceedance probability per row and constraint')
    z = NormalDist().inv_cdf(1.0 - float(prob))
    sig = report['sig_max']
    out = dict(z=z, disc=z * sig)
    if report.get('fence_sn') is not None:
        out['fence'] = z * report['fence_sn']
    if pair is not None:
        if report['gust'].form_corr > 0.0:
            raise NotImplementedError(f"pair margins with form_corr = {report['gust'].form_corr} > 0: the cross-covariance between two "
                                      'aircraft of a formation is not computed')
        i, j = pair
        out['pair'] = z * (sig[i] ** 2 + sig[j] ** 2) ** 0.5
    return out


def implement_controller(n_ac, time, x_ref, y_ref, v, w, X0s):
    """The reference's 6-tuple X_array, U_array, X_ref_array, Yd_ref_array, Ydd_ref_array, dX_array
    (src/11_full_sim_case1.py:241-291), each (T, n_ac, .)."""
    out = implement_controller_batch(time, x_ref, y_ref, w, X0s)
    d2dhip.default_context().sync()
    t = lambda k: out[k].cpu().numpy().transpose(0, 2, 1)      # noqa: E731
    return t('X'), t('U'), t('Xr'), t('Yd'), t('Ydd'), t('dX')


def _rows_select_pairs(scen_rows, n_ac):
    """True when the rows' partner sets (SC_PMASK) are anything but what the default lowering writes -- 0b10 / 0b01 (or nothing) on
    aircraft 0 and 1, nothing on the others: such rows are solved by d2d_nlp_solve_groups_pairs (multi_opt_planner.scenario_rows
    writes them for CostCollision(pairs=) / CostComposit(col_pairs=))."""
    pm = np.asarray(scen_rows, dtype=np.float64)[:, d2dhip.SC_PMASK].reshape(-1, n_ac)
    if n_ac < 2:
        return bool((pm != 0).any())
    return bool((~np.isin(pm[:, 0], (0, 0b10))).any() or (~np.isin(pm[:, 1], (0, 0b01))).any() or (pm[:, 2:] != 0).any())


def _moving_tables(ctx, moving, n_scen):
    """Device tables (knots [n_scen][n_mov][n_knot][3], disc [n_scen][n_mov][2]) of `moving`: a list of d2d.opty_utils.MovingObstacle
    that every scenario sees, or one such list per scenario (the same number of discs in each; an absent disc has r <= 0)."""
    import d2d.opty_utils as d2ou
    moving = list(moving)
    per = [list(m) for m in moving] if moving and not isinstance(moving[0], d2ou.MovingObstacle) else [moving] * n_scen
    if len(per) != n_scen or len({len(m) for m in per}) != 1:
        raise ValueError(f'moving obstacles: one list for all scenarios or one list per scenario ({n_scen}) with the same number of discs')
    n_knot = max(len(o.t) for m in per for o in m)
    tabs = [d2ou.lower_moving(m, n_knot) for m in per]
    return ctx.dev(np.stack([t[0] for t in tabs])), ctx.dev(np.stack([t[1] for t in tabs]))


def _hard_moving_tables(ctx, hard, rows, n_ac, h):
    """Device tables (knots [n_scen][n][n_knot][3], disc [n_scen][n][2] = (R, 1)) of `hard`: a list of d2d.opty_utils.MovingKeepOut /
    KeepOut that every scenario holds, or one such list per scenario (the same number of discs in each), lowered with the largest
    VMAX of the scenario's rows and h."""
    import d2d.opty_utils as d2ou
    n_scen = len(rows) // n_ac
    hard = list(hard)
    per = [list(m) for m in hard] if hard and not hasattr(hard[0], 'lowered') else [hard] * n_scen
    if len(per) != n_scen or len({len(m) for m in per}) != 1 or not per[0]:
        raise ValueError(f'hard_moving: one non-empty list for all scenarios or one list per scenario ({n_scen}) with the same number of discs')
    n_knot = max([len(o.t) for m in per for o in m if hasattr(o, 't')] + [2])
    vmax = rows[:, d2dhip.SC_VMAX].reshape(n_scen, n_ac).max(axis=1)
    tabs = [d2ou.lower_keep_moving(m, float(vmax[r]), h, n_knot) for r, m in enumerate(per)]
    return ctx.dev(np.stack([t[0] for t in tabs])), ctx.dev(np.stack([t[1] for t in tabs]))


def _via_table(dsc, n_ac, N, h, t_start, via):
    """plan_batch's timed waypoints: the table (B, n_via, 5) of every problem on its scenario's clock."""
    import d2d.opty_utils as d2ou
    B = dsc.shape[0]
    via = [list(v or []) for v in via]
    if len(via) != B:
        raise ValueError(f'via: one waypoint list per problem ({B})')
    ts = t_start.cpu().numpy() if hasattr(t_start, 'cpu') else np.full(B // n_ac, 0.0 if t_start is None else float(t_start))
    n_via = max(1, max(len(v) for v in via))
    return np.stack([d2ou.lower_waypoints(v, float(ts[b // n_ac]), h, N, n_via) for b, v in enumerate(via)])


def _dev_i32(ctx, v, n, name):
    """None, or (n,) integers as a device int32 tensor (a tensor is taken as it is)."""
    if v is None or hasattr(v, 'data_ptr'):
        return v
    a = np.asarray(v)
    if a.shape != (n,):
        raise ValueError(f'{name}: one integer per formation ({n}) is required, got shape {a.shape}')
    return ctx.dev(np.ascontiguousarray(a, dtype=np.int32))


def deconflict_plans(ctx, scen, W, h, n_ac, world=None, prio=None, row0=None, *, d_sep, margin, d_look, n_knot=32, n_mov=8, max_rounds=4,
                     field=None, t0=0.0, step_max=None, kind=1, hard=False, **solve_kw):
    """Prioritised re-planning of formations that share an airspace.  scen dev [R n_ac][SCEN_STRIDE] and W dev [R n_ac][5][N] are the
    rows and the plans of R formations of n_ac aircraft, from any collocation entry, node i of formation r at t0 + (row0[r] + i) h;
    world, prio, row0: (R,) integers or device int32 tensors (None: one world, the formation index, 0).  The formation with the smaller
    (prio, index) keeps its plan; the others give way.  Per round, on the device:
      1. the plans are viewed as a history [N][5][R n_ac] with dt_row = h;
      2. Context.fleet_tracks lists, per formation, up to n_mov aircraft of formations that outrank it and come within d_look, as
         moving discs of radius d_sep + margin + chord_err (what n_knot knots give away of the partner's path), kind `kind`;
      3. the formations that have such partners and whose tables can differ from those of their last solve -- solved for the first
         time, another set of partners, or a partner whose plan changed in the round before -- are gathered and re-solved around
         their discs from their current plan (nlp_solve_groups_moving; nlp_solve_moving when n_ac == 1) with t_start = t0 + row0 h;
         their number is the only scalar that visits the host;
      4. the solutions are scattered back; a formation whose re-solve does not converge keeps the plan it had and is reported.
    The loop ends when nothing is left to re-solve or after max_rounds.  (A formation that has given way still flies within d_look of
    the one it avoided, so "has partners" alone would never end; a formation none of whose partners moved is at its fixed point.)
    step_max (m): the longest step of any plan between two nodes, for the grid of fleet_tracks; None: h (max SC_VMAX + max |row wind|)
    x 1.05, read once before the first round (with a field it must be given).  solve_kw: the solver's keywords; bounds dev [R n_ac][4]
    are gathered with the rows.
    hard=False: the moving discs are a SOFT cost (the rows' KOBS and S weigh them) and the function reports the separation it reached.
    hard=True: the discs are HARD constraints of the re-solve (nlp_solve_groups_keepout; nlp_solve_keepout_moving when n_ac == 1), with
    the node radius R = sqrt((d_sep + margin)^2 + step_max^2) + chord_err, computed on the device; the rows' soft static discs still
    count, `kind` is not read.  step_max is the longest step of any plan between two nodes, so two aircraft move at most 2 step_max
    relative to each other between two rows, and a relative chord between two relative positions on the circle R passes the centre at
    sqrt(R^2 - step_max^2) >= d_sep + margin.  THE THEOREM: if truncated is false and not_converged, refused and unresolved are empty
    at a fixed point of the loop (rounds < max_rounds), every aircraft's continuous closest approach to every outranking aircraft
    within d_look is >= d_sep + margin.
    Returns W (changed in place) and info: rounds; replanned (formations re-solved, per round); solves (per round:
    dict(forms, cost, status, feas) of device tensors); truncated (some formation had more partners than n_mov in some round);
    not_converged (formation indices); refused (hard=True: formations whose re-solve was refused on the device -- e.g. an outranking
    aircraft inside R of their pinned start pose; they keep their plan, like not_converged; else []); tracks_status (dev int32 [R] of the last round); audit: the final Context.fleet_audit
    (near_dist, near_partner, ... with d_safe = d_sep); unresolved: the formations with an aircraft still below d_sep."""
    import torch                    # (tensor plumbing on the device of W; everything computed goes through ctx)
    n_ac, n_mov, n_knot = int(n_ac), int(n_mov), int(n_knot)
    B, _, N = W.shape
    R = B // n_ac
    if R * n_ac != B or scen.shape[0] != B:
        raise ValueError(f'deconflict_plans: {B} plans and {scen.shape[0]} rows are not whole formations of {n_ac}')
    h, t0, r_disc = float(h), float(t0), float(d_sep) + float(margin)
    world, prio, row0 = (_dev_i32(ctx, v, R, k) for v, k in ((world, 'world'), (prio, 'prio'), (row0, 'row0')))
    if step_max is None:
        if field is not None:
            raise ValueError('deconflict_plans: with a wind field step_max (the longest step between two nodes, m) must be given')
        step_max = 1.05 * h * float((scen[:, d2dhip.SC_VMAX].max() + torch.hypot(scen[:, d2dhip.SC_WX], scen[:, d2dhip.SC_WY]).max()).item())
    bounds = solve_kw.pop('bounds', None)
    t_start = torch.full((R,), t0, dtype=torch.float64, device=W.device)
    if row0 is not None:
        t_start = t_start + row0.to(torch.float64) * h
    ac = torch.arange(n_ac, device=W.device)
    last_set = torch.full((R, n_mov), -2, dtype=torch.int32, device=W.device)       # the partners a formation was last solved against
    changed = torch.zeros(R, dtype=torch.bool, device=W.device)                       # plans that the round before replaced
    bad = torch.zeros(R, dtype=torch.bool, device=W.device)
    refused = torch.zeros(R, dtype=torch.bool, device=W.device)
    if hard:
        r_disc = float(np.sqrt(r_disc ** 2 + float(step_max) ** 2))
    trunc = torch.zeros((), dtype=torch.bool, device=W.device)
    replanned, solves, tr = [], [], None
    fleet_kw = dict(row0=row0, world=world)
    for _ in range(int(max_rounds)):
        tr = ctx.fleet_tracks(W.permute(2, 1, 0).contiguous(), n_ac, h, float(d_look), step_max, r_disc, prio=prio, n_mov=n_mov, n_knot=n_knot,
                              kind=kind, t0=t0, **fleet_kw)
        partner, n_conf, disc = tr['partner'], tr['n_conf'], tr['disc']
        disc[:, :, 0] += torch.where(partner >= 0, tr['chord_err'], torch.zeros_like(tr['chord_err']))
        trunc |= (n_conf == n_mov + 1).any()
        pset = torch.sort(partner, dim=1).values
        moved = (changed[torch.clamp(partner, min=0) // n_ac] & (partner >= 0)).any(dim=1)
        forms = torch.nonzero((n_conf > 0) & (moved | (pset != last_set).any(dim=1))).flatten()
        n = int(forms.numel())                                                        # the round's one scalar on the host
        if n == 0:
            break
        sel = (forms[:, None] * n_ac + ac[None, :]).flatten()
        Wg = W[sel].contiguous()
        args = (scen[sel].contiguous(), Wg, h)
        kw = dict(knots=tr['knots'][forms].contiguous(), disc=disc[forms].contiguous(), field=field, t_start=t_start[forms].contiguous(),
                  **({} if bounds is None else dict(bounds=bounds[sel].contiguous())), **solve_kw)
        if hard:
            res = ctx.nlp_solve_keepout_moving(*args, **kw) if n_ac == 1 else ctx.nlp_solve_groups_keepout(*args, n_ac, **kw)
        else:
            res = ctx.nlp_solve_moving(*args, **kw) if n_ac == 1 else ctx.nlp_solve_groups_moving(*args, n_ac, **kw)
        ok = (res['status'] == d2dhip.ST_CONVERGED).view(n, n_ac).all(dim=1)
        W[sel] = torch.where(ok.repeat_interleave(n_ac)[:, None, None], Wg, W[sel])
        changed = torch.zeros_like(changed)
        changed[forms] = ok
        bad[forms] = ~ok
        if hard:
            refused[forms] = (res['status'] == d2dhip.ST_NONFINITE).view(n, n_ac).any(dim=1)
            bad[forms] &= ~refused[forms]
        last_set[forms] = pset[forms]
        replanned.append(n)
        solves.append(dict(forms=forms, cost=res['cost'], status=res['status'], feas=res['feas']))
    audit = ctx.fleet_audit(W.permute(2, 1, 0).contiguous(), n_ac, h, float(d_look), step_max, d_safe=float(d_sep), **fleet_kw)
    low = (audit['near_dist'] < float(d_sep)).view(R, n_ac).any(dim=1)
    info = dict(rounds=len(replanned), replanned=replanned, solves=solves, truncated=bool(trunc.item()),
                not_converged=[int(f) for f in torch.nonzero(bad).flatten().cpu()],
                refused=[int(f) for f in torch.nonzero(refused).flatten().cpu()], tracks_status=None if tr is None else tr['status'],
                audit=audit, unresolved=[int(f) for f in torch.nonzero(low).flatten().cpu()])
    return W, info


def _start_nodes(ctx, dsc, K, h, W0, bounds):
    """The start of a collocation solve on the device: W0 an array (B, 5, K) of node values, or 'dubins' -- every row's Dubins path,
    built there from the rows (d2d_nlp_guess_dubins).  -> W (device), the guess's status (device int32 [B]; None for an array)."""
    if isinstance(W0, str):
        if W0 != 'dubins':
            raise ValueError(f"W0={W0!r}: an array (B, 5, K) of node values or 'dubins'")
        W, g = ctx.nlp_guess_dubins(dsc, K, h, bounds=bounds, outputs=('status',))
        return W, g['status']
    return ctx.dev(np.ascontiguousarray(W0, dtype=np.float64)), None


def _keep_table(keep_out, rows, steps):
    """keep_out -> the table (B, n, 3) of (cx, cy, R) that the kernel reads: an array is taken as it is; a list of d2d.opty_utils.KeepOut is
    lowered per problem with the row's VMAX and that problem's step steps[b] (a free step: the largest one of its box)."""
    B = len(rows)
    if len(keep_out) and hasattr(keep_out[0], 'lowered'):
        import d2d.opty_utils as d2ou
        return np.stack([d2ou.lower_keep_out(keep_out, rows[b, d2dhip.SC_VMAX], steps[b]) for b in range(B)])
    keep = np.ascontiguousarray(keep_out, dtype=np.float64)
    if keep.ndim != 3 or keep.shape[0] != B or keep.shape[2] != 3:
        raise ValueError(f'keep_out: an array (B, n, 3) of (cx, cy, R) or a list of KeepOut is required, got shape {keep.shape}')
    return keep


def _fence_table(fence, G):
    """fence -> the table (G, n, 4) of (ax, ay, b, kap): one d2d.opty_utils.GeoFence for all G scenarios, one per scenario, or the rows."""
    import d2d.opty_utils as d2ou
    if isinstance(fence, d2ou.GeoFence):
        return np.stack([fence.lowered()] * G)
    if isinstance(fence, (list, tuple)) and len(fence) and isinstance(fence[0], d2ou.GeoFence):
        if len(fence) != G or len({len(f.a) for f in fence}) != 1:
            raise ValueError(f'fence: one GeoFence for all scenarios or one per scenario ({G}) with the same number of edges')
        return np.stack([f.lowered() for f in fence])
    ftab = np.ascontiguousarray(fence, dtype=np.float64)
    if ftab.ndim != 3 or ftab.shape[0] != G or ftab.shape[2] != 4:
        raise ValueError(f'fence: a GeoFence, a list of them or an array ({G}, n, 4) of (ax, ay, b, kap) is required, got shape {ftab.shape}')
    return ftab


def _default_pair_rows(dsc, n_ac, pairs, clone=True):
    """The rows as the group entries that read partner sets want them: the reference's pair (0, 1) written as SC_PMASK of the coupled
    scenarios -- into a copy, or with clone=False into dsc itself -- unless there is one aircraft or the rows select their pairs
    (`pairs`, _rows_select_pairs): then dsc as it is."""
    if n_ac < 2 or pairs:
        return dsc
    out = dsc.clone() if clone else dsc
    d2mou.default_pair_masks(out, n_ac, (out[0::n_ac, d2dhip.SC_KCOL] > 0) & (out[1::n_ac, d2dhip.SC_KCOL] > 0))
    return out


# plan_batch's optional features in the order they are looked at -> what the polynomial fit lacks and what backend='nlp' does with it ...
PLAN_BATCH_FIT = {
    'moving': ('moving obstacles', 'plans around them'), 'via': ('timed waypoints', 'plans through them'), 'windfield': ('wind field', 'plans in one'),
    'free_time': ('free time step', 'plans with one'), 'window': ('free time step', 'plans with one (fit backend)'),
    'keep_out': ('hard keep-out discs', 'holds them'), 'fence': ('geofence', 'holds one'), 'hard_moving': ('hard moving discs', 'holds them'),
    'deconflict': ('deconfliction', 're-plans by priority')}
# ... and the features each refuses beside it (the first one given is the one named), with the reason.  (free_time's two sentences are
# its own, in plan_batch; fence with keep_out and n_ac > 1 is keep_out's to refuse.)
PLAN_BATCH_REFUSES = {
    'window': (('n_ac > 1', 'windfield', 'moving', 'via', 'hard_moving', 'deconflict', 'free_time'),
               'a free step beside static hard discs and a geofence is held for one aircraft in the rows\' constant wind, without pins or '
               'anything that moves'),
    'keep_out': (('n_ac > 1', 'moving', 'via', 'free_time'), 'hard discs are held for one aircraft on static discs, without pins, with a fixed step'),
    'fence': (('moving', 'via', 'free_time', 'hard_moving', 'deconflict'),
              'a geofence is held with static hard discs for one aircraft, without them for several, without moving discs or pins, with a fixed step'),
    'hard_moving': (('moving', 'via', 'free_time', 'keep_out', 'deconflict'),
                    'hard moving discs go with neither soft moving discs, pins, a free step nor static hard discs (list a KeepOut in '
                    'hard_moving), and the re-solve of deconflict does not carry them'),
    'deconflict': (('free_time', 'keep_out', 'via', 'moving'),
                   'the re-solve around the committed plans (d2d_nlp_solve_groups_moving) does not carry {name}')}


def plan_batch(scen_rows, K, duration, obj_scale_over_n, q0=None, backend='fit', W0=None, h=None, n_ac=1, windfield=None, t_start=0.0,
               moving=None, via=None, gust=None, free_time=None, kdur=0.0, keep_out=None, deconflict=None, hard_moving=None, fence=None, window=None, **solve_kw):
    """Batched planning entry point: scen_rows (B, d2dhip.SCEN_STRIDE) in the d2dhip layout -> dict with device
    tensors q, cost, iters, status and host stats (polynomial fit, backend='fit').
    backend='nlp': the reference's direct-collocation Problem (hard bounds) for B / n_ac scenarios of n_ac aircraft in one launch
    (d2d_nlp_solve_groups; CostCollision couples aircraft 0 and 1 of a scenario whose rows carry KCOL > 0): W0 (B, 5, K) node
    values of the initial guess, h the time step -> dict with device tensors W (the solution), cost, feas, iters, status per
    aircraft and sweeps, moved per scenario.  W0='dubins' (backend='nlp'): every row's start is its Dubins path, built on the device
    from the row (d2d_nlp_guess_dubins: the row's constant wind, solve_kw's bounds; each aircraft of a scenario on its own; discs and a
    field are not seen) -- the result gains guess_status (device int32 [B], d2dhip.GUESS_STATUS; a refused row starts from zeros and
    its solve says so); not with via=.  windfield (backend='nlp'): a SplineWindField the problems are planned in, AS GIVEN -- it is the
    planner's field, whose model adds it to the residual, so a plan for a plant that flies F takes -F -- with node i of scenario r at
    t_start[r] + i h (d2d_nlp_solve_groups_wind); t_start a float or a device tensor [B / n_ac]; the rows' wind columns are not read.
    Rows whose SC_PMASK name other partners than the pair (0, 1) (multi_opt_planner.scenario_rows for a cost with `pairs`) are solved
    by d2d_nlp_solve_groups_pairs, with and without a field.
    moving (backend='nlp'): moving obstacles -- a list of d2d.opty_utils.MovingObstacle for all scenarios or one list per scenario --
    that every aircraft plans around, node i of scenario r at t_start[r] + i h, with the rows' KOBS and S as their weight
    (d2d_nlp_solve_groups_moving, with and without a field).
    via (backend='nlp'): timed waypoints -- one list of d2d.opty_utils.Waypoint per PROBLEM (row of scen_rows; an empty list: no pin) --
    on the clock of t_start, held exactly (d2d_nlp_solve_groups_via, with and without a field or moving obstacles); the result carries
    via (the device table) and waypoint_error, the largest |plan - pin|: 0.0.  Like moving=, via= goes through the group entry
    for every n_ac: with n_ac = 1 that is one workgroup with one wavefront per problem, each with its own workspace, not the persistent
    hand-out of d2d_nlp_solve_via -- for large batches of single aircraft call Context.nlp_solve_via (the difference is not measured).
    free_time (backend='nlp', n_ac = 1): (h_lo, h_hi) for all problems or an array (B, 2) -- every problem's time step is an unknown in
    that box, started from h, with kdur (a number or (B,)) the weight of the duration (K - 1) h in its objective (d2d_nlp_solve_free);
    the result carries h, the solved steps (device [B]).
    keep_out (backend='nlp', n_ac = 1): hard keep-out discs -- an array (B, n, 3) of (cx, cy, R), the node constraint as the kernel reads
    it, or a list of d2d.opty_utils.KeepOut for all problems, lowered with each row's VMAX and h (d2d_nlp_solve_keepout, with and
    without a field); the result carries keep_mult (device [B][n][K]) and keep (the lowered table, a host array (B, n, 3)).
    hard_moving (backend='nlp', any n_ac): hard keep-out discs that MOVE -- a list of d2d.opty_utils.MovingKeepOut (and KeepOut) for all
    scenarios or one list per scenario -- that every aircraft of the scenario holds, node i at t_start[r] + i h, lowered with the
    scenario's largest VMAX and h (d2d_nlp_solve_groups_keepout; d2d_nlp_solve_keepout_moving when n_ac = 1; with and without a field);
    the result carries keep_mult (device [B][n][K]) and hard_knots, hard_disc (the lowered device tables).
    fence (backend='nlp', any n_ac): a hard geofence -- one d2d.opty_utils.GeoFence for all scenarios, one per scenario (a list of
    B / n_ac), or the lowered rows, an array (B / n_ac, n, 4) of (ax, ay, b, kap) -- that every aircraft's plan stays inside, its polyline
    included (n_ac = 1: d2d_nlp_solve_fence, with and without keep_out's static hard discs in the same solve; n_ac > 1:
    d2d_nlp_solve_groups_fence, which carries no hard discs; both with and without a field); the result carries fence_mult (device
    [B][n][K]) and fence (the lowered table, a host array).
    window (backend='nlp', n_ac = 1): free_time's box -- (h_lo, h_hi) for all problems or an array (B, 2), with kdur -- for a plan that also
    holds keep_out's static hard discs and a fence (either, both or neither) in the same solve (d2d_nlp_solve_free_fence): the spelling
    of a free step beside hard constraints (free_time keeps refusing them).  A list of KeepOut is lowered with each row's VMAX and the
    LARGEST step of its box, h_hi: conservative for every step the solve may end at; the fence is convex and needs none.  The result
    carries h and free_rows as free_time's, keep / keep_mult and fence / fence_mult as keep_out's and fence's.
    deconflict (backend='nlp'): None -- today's call, bit for bit -- or a dict of deconflict_plans' keywords (d_sep, margin, d_look
    required; world, prio, n_knot, n_mov, max_rounds, step_max, kind, hard): after the solve the formations (the scenarios) that share a
    world give way to each other by priority (deconflict_plans, which re-solves with this call's solve_kw, in the field and from the
    start times of this call); W is updated in place and the result carries deconflict, its info.  Start times must be whole multiples
    of h apart (fleet_row0 names the formation that is not).
    What does not combine is refused by name (NotImplementedError), from PLAN_BATCH_FIT and PLAN_BATCH_REFUSES -- the feature on the left
    is not planned together with those on the right; none of them, nor windfield, moving or via, with the fit backend:
      free_time    n_ac > 1, windfield, moving, via
      window       n_ac > 1, windfield, moving, via, hard_moving, deconflict, free_time
      keep_out     n_ac > 1, moving, via, free_time
      fence        moving, via, free_time, hard_moving, deconflict
      hard_moving  moving, via, free_time, keep_out, deconflict
      deconflict   free_time, keep_out, via, moving"""
    import single_opt_planner as sop
    from d2d.wind import planner_wind
    if gust is not None:
        raise ValueError('a gust is a property of the plant, not of a plan: the planners take none (fly the plan through it with '
                         'implement_controller_batch(gust=...) or full_sim_phases_batch(gust=...))')
    fld = planner_wind(windfield)
    given = {'n_ac > 1': int(n_ac) != 1, 'windfield': fld is not None, 'moving': bool(moving), 'via': via is not None, 'free_time': free_time is not None,
             'keep_out': keep_out is not None, 'deconflict': deconflict is not None, 'hard_moving': hard_moving is not None,
             'fence': fence is not None, 'window': window is not None}
    given = {k for k, g in given.items() if g}
    if backend != 'nlp':
        for name, (what, does) in PLAN_BATCH_FIT.items():
            if name in given:
                raise NotImplementedError(f"the polynomial fit has no {what}: plan_batch(backend='nlp', {name}=...) {does}")
    if 'free_time' in given:                      # (its two sentences fit no row: one for n_ac, one that names three features)
        if 'n_ac > 1' in given:
            raise NotImplementedError('free_time with n_ac > 1: the aircraft of a scenario share one time step, which the block '
                                      'Gauss-Seidel over the aircraft cannot hold; plan them one at a time')
        if given & {'windfield', 'moving', 'via'}:
            raise NotImplementedError('free_time together with windfield, moving or via is not supported: node times move with the step')
    for lead, (names, why) in PLAN_BATCH_REFUSES.items():
        if lead in given:
            for name in names:
                if name in given:
                    raise NotImplementedError(f'{lead} with {name} is not supported: ' + why.format(name=name))
    if deconflict is not None:
        deconflict = dict(deconflict)
        unknown = set(deconflict) - {'d_sep', 'margin', 'd_look', 'world', 'prio', 'n_knot', 'n_mov', 'max_rounds', 'step_max', 'kind', 'hard'}
        missing = {'d_sep', 'margin', 'd_look'} - set(deconflict)
        if unknown or missing:
            raise ValueError(f'deconflict: needs d_sep, margin and d_look and takes world, prio, n_knot, n_mov, max_rounds, step_max, kind '
                             f'(unknown: {sorted(unknown)}, missing: {sorted(missing)})')
        n_scen = len(scen_rows) // int(n_ac)
        ts = t_start.cpu().numpy() if hasattr(t_start, 'cpu') else np.full(n_scen, float(t_start))
        dec_row0 = fleet_row0(ts, float(h))                 # refuses an off-grid start by name, before anything is solved
        dec_t0 = float(ts.min())
    ctx = d2dhip.default_context()
    if backend == 'nlp':
        if window is not None and h is None:
            raise ValueError('plan_batch(window=): h, the start step, is required')
        rows = np.ascontiguousarray(scen_rows, dtype=np.float64)
        dsc = ctx.dev(rows)
        assert h is not None
        B, h, n_ac = rows.shape[0], float(h), int(n_ac)
        if isinstance(W0, str) and W0 == 'dubins' and via is not None:
            raise NotImplementedError("W0='dubins' with via=: a Dubins path knows no pins; the 'via' guess does "
                                      "(d2d.opty_utils.via_guess, Planner.get_initial_guess('via')): pass its node values as W0")
        W, guess_status = _start_nodes(ctx, dsc, K, h, W0, solve_kw.get('bounds'))      # ('dubins': built on the device from the rows, no host copy)
        assert W.shape == (B, 5, K)
        step = window if window is not None else free_time
        # one aircraft with a hard family or a free step: the hand-out entries; everything else the group entries, for every n_ac (the
        # docstring's note on via= with n_ac = 1)
        hand = n_ac == 1 and any(v is not None for v in (step, keep_out, fence, hard_moving))
        pairs = _rows_select_pairs(scen_rows, n_ac)          # partner sets other than the reference's pair (0, 1)
        host, dev, mov = {}, {}, {}                          # lowered tables: host arrays and device tensors the result carries; the discs' tracks
        if step is not None:
            fr = np.zeros((B, 4))
            fr[:, :2] = np.broadcast_to(np.asarray(step, dtype=np.float64), (B, 2))
            fr[:, 2] = np.broadcast_to(np.asarray(kdur, dtype=np.float64), (B,))
            host['free_rows'] = fr
        if keep_out is not None:                             # (a free step: the chord term at the largest step of the box)
            host['keep'] = _keep_table(keep_out, rows, np.full(B, h) if window is None else fr[:, 1])
        if fence is not None:
            host['fence'] = _fence_table(fence, B // n_ac)
        if hard_moving is not None:
            dev['hard_knots'], dev['hard_disc'] = _hard_moving_tables(ctx, hard_moving, rows, n_ac, h)
        if via is not None:
            table = _via_table(dsc, n_ac, K, h, t_start, via)
            dev['via'] = ctx.dev(table)
        if moving:
            mov['knots'], mov['disc'] = _moving_tables(ctx, moving, B // n_ac)
        scen = dsc
        if fence is not None or hard_moving is not None or via is not None:      # their group entries read the partner sets
            scen = _default_pair_rows(dsc, n_ac, pairs, clone=via is None)       # (via= writes them into the rows it returns)
        if fld is None and not moving and (via is not None or keep_out is not None or fence is not None):
            t_start = None                                   # (no clock but the pins', whose table is on it already)
        spelt = {'free_rows': 'window'} if window is not None else {}       # (nlp_plan's spelling of a free step beside hard constraints)
        out = d2dhip.nlp_plan(ctx, scen, W, h, n_ac=None if hand else n_ac, field=fld, t_start=t_start, pairs=pairs, **mov, **dev,
                              **{spelt.get(k, k): ctx.dev(v) for k, v in host.items()}, **solve_kw)
        out.update(host, **dev)
        if via is not None:
            import d2d.opty_utils as d2ou
            ctx.sync()
            Wh = W.cpu().numpy()
            out['waypoint_error'] = max(d2ou.waypoint_error(table[b], Wh[b]) for b in range(len(Wh)))
        if deconflict is not None:                           # (the re-solve entry reads the partner sets too)
            _, out['deconflict'] = deconflict_plans(ctx, _default_pair_rows(dsc, n_ac, pairs), W, h, n_ac, row0=dec_row0, field=fld, t0=dec_t0,
                                                    **deconflict, **solve_kw)
        out.update(W=W, scen=dsc)
        if guess_status is not None:
            out['guess_status'] = guess_status
        return out
    if isinstance(W0, str):
        raise NotImplementedError(f"W0={W0!r} is a start of the collocation backend (backend='nlp'): the polynomial fit starts from q0")
    plan = sop.get_plan(K, duration, obj_scale_over_n)
    dsc = ctx.dev(np.ascontiguousarray(scen_rows, dtype=np.float64))
    q = plan.init(dsc) if q0 is None else q0
    cost, iters, status, stats = plan.solve(dsc, q, **solve_kw)
    return dict(plan=plan, scen=dsc, q=q, cost=cost, iters=iters, status=status, stats=stats)


def full_sim_phases_batch(c, r, v, n_ac, X1_f, scen, X2_f, t_opt, ref3=None, t_sim_end=200., w=(0., 0.), t_step=0.05,
                          t_end_1=1000., X0=None, max_sweeps=250, record2=('X', 'U'), record3=('X', 'U'), windfield=None,
                          moving_obstacles=None, audit=None, gust=None, gust_stream_base=0, wind_estimate=None):
    """The three phases of src/11_full_sim_case1.py main() (:406-478) for many independent formations, chained ON THE
    DEVICE: the circular-formation phase hands its final states to the planner as a device tensor, the planner's sampled
    plan is the tracking reference of phase 2 without leaving HBM, and phase 3 restarts from phase 2's final states.

      c (n_form, n_ac, 2) centres, r radius, v flight speed, X1_f (n_ac, >=3) or (n_form, n_ac, >=3) the formation
      that ends phase 1 (:421)
      scen        multi_opt_planner scenario class (trap_4, :444); its p0s come from phase 1, p1s = X2_f ((n_ac, >=3) or
                  (n_form, n_ac, >=3)), t1 = t_opt
      ref3        (time_3, x_ref_3, y_ref_3) of phase 3 -- e.g. ExtendTraj_symm(ExtractTrajData(csv)) -- or None
    Returns a dict of device tensors (plane-major, drone index = formation * n_ac + aircraft):
      phase1 (gvf_run dict), plan (q, cost, Xs [N][5][K]), phase2 (track_run dict), phase3 (list of track_run dicts).
    windfield: a SplineWindField F the PLANT flies through all three phases; None (or a constant class): the constant w, the chain
    above.  In a field the chain differs in this:
      phase 1   flies F (row i at i t_step);
      the plan  starts, per formation, at the time its phase 1 ended, t2[r] = (min(stop_row[r], rows) - 1) t_step (computed on the
                device), and is the collocation problem of all aircraft of the formation IN -F (the model adds its wind to the residual:
                a plan consistent with a plant that flies F is planned in -F), collision pair included -- d2d_nlp_solve_groups_wind.
                Its initial guess is the polynomial fit of the constant chain, each row's constant wind set to the field at that
                aircraft's own start pose and time, sampled at the nodes: the fit proposes, the collocation problem decides (as
                Planner._harden);
      phase 2   tracks the plan's x, y node planes in F, every drone from its formation's t2; phase 3 likewise, repetition k from
                t2 + dur2 + k time_3[-1].
    No state visits the host between the phases.  plan gains W (= Xs, now the collocation plan [N][5][K]), cost_fit, feas, status,
    iters, sweeps, moved, t_start [n_form] and field (-F, F.negated(): the planner's field; the entry also keeps its device copy
    alive while the launches that read it are queued); plan['q'] is the fit's (the guess); the controllers keep the constant w.
    A scen.cost that selects its own collision pairs (CostComposit(col_pairs=...)): the fit couples those pairs (SC_PMASK) and the
    plan is the collocation problem over all of them (d2d_nlp_solve_groups_pairs), in -F or, without a field, in the rows' constant
    wind; plan gains `pairs` and, without a field too, W, cost_fit, feas, status, iters, sweeps, moved.
    moving_obstacles: a list of d2d.opty_utils.MovingObstacle (or one list per formation) on the mission's clock.  Each formation's
    transition is the collocation problem around them from that formation's own end-of-phase-1 time t2[r] (the device array above,
    computed with or without a field), in -F or in the rows' constant wind (d2d_nlp_solve_groups_moving), from the fit's plan as the
    guess; the weight is scen.cost's kobs.  plan gains the entries listed for a field, t_start included, and mov_work: the discs'
    centres at the plan's nodes [n_form][n_mov][2][K].
    audit: None (nothing is launched, the result is what it was), True or a dict (d_safe, err_tol, static: _audit_kw).  out['audit']
    then holds Context.flight_audit dictionaries of what was planned and what was flown: plan (the plan Xs as a history with
    dt_row = dt2), phase2 (the flown X against the plan's x, y) and phase3 (a list, one per repetition, against the phase-3
    reference) -- on the chain's clock where it has one (a field or moving discs: t_start = t2, repetition k of phase 3 from
    t2 + dur2 + k time_3[-1]) and around the chain's moving discs.  'X' must be in record2 / record3.  With fleet=dict(d_look=,
    step_max=, world=...) in the dict every one of these dictionaries gains 'fleet': Context.fleet_audit of the same plan or history
    across the formations.  Every formation starts its transition when ITS phase 1 ended, t2[f] (in every chain, with or without a
    field), so formation f is placed at row0 = (t2[f] - min t2) / dt_row (read on the host; a formation more than 1e-9 rows off the
    common grid: ValueError naming it -- fleet_row0; the repetitions of phase 3 keep the same offsets on their own dt_row).
    gust: None (nothing new is launched, the result is what it was) or a d2d.wind.GustModel the PLANT flies through all three phases
    on top of w or F -- an unmeasured disturbance: neither the controllers nor the plan see it.  Every loop counts its steps from 1
    under its own phase word (phase 1: 0, phase 2: 1, repetition k of phase 3: 2 + k) and hands its gust state to the next on the
    device (phase*['gust_state'] dev [4][N]; 'g' in record2 / record3 keeps the flown gusts); gust_stream_base: the global index of the
    first drone when the formations are a shard of a larger study.
    wind_estimate: None (every path above, bit for bit) or a d2d.wind.WindEstimator -- the planner is no longer handed the truth.  Phase 1
    keeps its state history on the device at the estimator's rec_stride, the field F^ is fitted to it (d2d_wind_fit, rows = the
    formations' stop rows) and the transition is planned in -F^ instead of -F (d2d_nlp_solve_groups_wind, or with moving_obstacles that
    path's field form), the fit's rows taking F^ at each aircraft's start; phases 2 and 3 fly the true windfield (or the constant w).
    No state visits the host between the phases.  out['wind_fit']: dict(estimate: the WindEstimate, stats dev [8], support dev,
    rms = (rms_x, rms_y), read when every launch is queued); plan['field'] is -F^."""
    import multi_opt_planner as mop
    if audit is not None and ('X' not in record2 or (ref3 is not None and 'X' not in record3)):
        raise ValueError("audit needs the flown histories: 'X' must be in record2 and record3")
    if getattr(scen, 'fence', None) is not None:
        raise NotImplementedError('the mission chain has no geofence (scen.fence): its transit is the multi-aircraft fit; plan one aircraft '
                                  "with plan_batch(backend='nlp', fence=...) (d2d_nlp_solve_fence)")
    if getattr(scen, 'keep_out', None):
        raise NotImplementedError('the mission chain has no hard keep-out discs (scen.keep_out): its transit is the multi-aircraft fit; plan '
                                  'one aircraft with single_opt_planner.Planner (d2d_nlp_solve_keepout)')
    import d2d.opty_utils as d2ou
    F = plant_wind(windfield)
    gust = plant_gust(gust)
    est = wind_estimator(wind_estimate)

    def gk(phase, state, track=False):
        """the gust arguments of the loop with this phase word (track: of Context.track_run, which is told the formation size)"""
        if gust is None:
            return {}
        return dict(gust=gust, gust_state=state, gust_phase=phase, gust_stream_base=gust_stream_base, **(dict(gust_n_ac=n_ac) if track else {}))

    ctx = d2dhip.default_context()
    torch = d2dhip._torch()
    c = np.asarray(c, dtype=np.float64).reshape(-1, n_ac, 2)
    n_form = c.shape[0]
    X1f = np.broadcast_to(np.asarray(X1_f, dtype=np.float64).reshape(-1, n_ac, np.shape(X1_f)[-1])[:, :, :3], (n_form, n_ac, 3))
    X2f = np.broadcast_to(np.asarray(X2_f, dtype=np.float64).reshape(-1, n_ac, np.shape(X2_f)[-1])[:, :, :3], (n_form, n_ac, 3))
    ph1 = CircularFormationGVF_batch(c, r, v, n_ac, X0f=X1f, t_step=t_step, t_end=t_end_1, X0=X0, windfield=F, **gk(0, None),
                                     **(dict(record=()) if est is None else dict(record=('X',), rec_stride=est.rec_stride, wind_estimate=est)))
    known = F if est is None else ph1['wind_estimate']            # what the planner knows of the field the plant flies
    Xs1 = ph1['X_final']                                            # dev [5][N]: state at each formation's stop row
    # ---- phase 2: plan from where phase 1 ended (scenario rows finished on the device) ----
    scen.t1 = t_opt
    N2, dt2, dur2 = d2ou.planner_timing(scen.t0, scen.t1, scen.hz)
    rows, plan, coupled = mop.scenario_rows(scen, [(0., 0., 0., 0., 0.)] * n_ac, X2f[0], N2, dur2, scen.obj_scale, scen.wind.w)
    rows = np.tile(rows, (n_form, 1))
    rows[:, [d2dhip.SC_X1, d2dhip.SC_Y1, d2dhip.SC_PSI1]] = X2f.reshape(-1, 3)
    dsc = ctx.dev(rows)
    dsc[:, d2dhip.SC_X0], dsc[:, d2dhip.SC_Y0], dsc[:, d2dhip.SC_PSI0] = Xs1[0], Xs1[1], Xs1[2]
    moving = list(moving_obstacles or [])
    fleet = audit is not None and audit is not True and audit.get('fleet') is not None
    if known is not None or moving or fleet:
        t2 = (torch.clamp(ph1['stop_row'], max=len(ph1['time'])) - 1).to(torch.float64) * float(t_step)      # dev [n_form]
    if fleet:               # refuse an off-grid formation before anything is planned or flown for it
        for dt_row in [dt2] + ([] if ref3 is None else [ref3[0][1] - ref3[0][0]]):
            fleet_row0(t2.cpu().numpy(), float(dt_row))
    if known is not None:
        t2d = t2.repeat_interleave(n_ac).contiguous()                                                       # dev [N]: per drone
        w0 = ctx.wind_sample(known, t2d, Xs1[:2].contiguous())         # (the rows store -w of the planner's wind: -(-F) = F)
        dsc[:, d2dhip.SC_WX], dsc[:, d2dhip.SC_WY] = w0[0], w0[1]
    q = plan.init(dsc)
    if coupled:
        try:
            cost, sweeps, stats = plan.solve_groups(dsc, q, n_ac, max_sweeps=max_sweeps, inner_iters=8)
        finally:
            plan.set_groups(1)
    else:
        cost, iters, status, stats = plan.solve(dsc, q)
    _, Xs = plan.sample(dsc, q)                                     # dev [N][5][K]
    pl = dict(q=q, cost=cost, Xs=Xs, scen=dsc, stats=stats)
    ac = ddyn.Aircraft()
    kw = dict(w=(float(w[0]), float(w[1])), tau_phi=ac.tau_phi, tau_v=ac.tau_v)
    kw2 = {}
    pairs = mop.scenario_pairs(scen, n_ac)                          # None: the reference's pair (0, 1), the chain as it was
    if moving or known is not None or pairs is not None:
        # the fit was the guess, the collocation problem decides: around the discs from t2, in -F from t2, over a cost's own pairs
        Fp = None if known is None else (F.negated() if est is None else known.negated_device_field(ctx))
        Xs = Xs.contiguous().clone()
        knots, disc = _moving_tables(ctx, moving, n_form) if moving else (None, None)
        sol = d2dhip.nlp_plan(ctx, dsc, Xs, float(dt2), n_ac=n_ac, knots=knots, disc=disc, field=Fp, t_start=t2 if (moving or known is not None) else None,
                              pairs=pairs is not None)
        pl.update(cost_fit=cost, cost=sol['cost'], Xs=Xs, W=Xs, feas=sol['feas'], status=sol['status'], iters=sol['iters'],
                  sweeps=sol['sweeps'], moved=sol['moved'])
        if moving or known is not None:
            pl['t_start'] = t2
        if moving:
            pl.update(mov_work=sol['mov_work'], moving=(knots, disc))
        if known is not None:
            pl['field'] = Fp
        if F is not None:
            kw['wind'] = F
            kw2 = dict(t_start=t2d)
    if pairs is not None:
        pl['pairs'] = pairs
    x_ref2 = Xs[:, 0, :].t().contiguous(); y_ref2 = Xs[:, 1, :].t().contiguous()     # dev [K][N]
    gs = ph1.get('gust_state')
    ph2 = ctx.track_run(x_ref2, y_ref2, Xs1, float(dt2), record=record2, **kw, **kw2, **gk(1, gs, track=True))
    gs = ph2.get('gust_state')
    out = dict(phase1=ph1, plan=pl, phase2=ph2, phase3=[])
    if audit is not None:
        akw = _audit_kw(ctx, audit, n_form, ('fleet',))
        if moving:
            akw.update(knots=pl['moving'][0], disc=pl['moving'][1])
        t2a = t2 if (F is not None or moving) else None
        out['audit'] = dict(plan=ctx.flight_audit(Xs, n_ac, float(dt2), t_start=t2a, layout='plan', **akw),
                            phase2=ctx.flight_audit(ph2['X'], n_ac, float(dt2), t_start=t2a, x_ref=x_ref2, y_ref=y_ref2, **akw), phase3=[])
        for key, hist, lay in (('plan', Xs, 'plan'), ('phase2', ph2['X'], 'hist')):
            if fleet:       # every formation's transition starts where ITS phase 1 ended, with or without a clock of the chain
                out['audit'][key]['fleet'] = _fleet_audit(ctx, audit, hist, n_ac, float(dt2), n_form, t_start=t2, layout=lay)
    # ---- phase 3: the periodic formation-flight reference, restarted from the last state until t_sim_end (:466-474) ----
    if ref3 is not None:
        time_3, x3, y3 = ref3
        x3 = ctx.dev(np.tile(np.ascontiguousarray(x3, dtype=np.float64), (1, n_form)))
        y3 = ctx.dev(np.tile(np.ascontiguousarray(y3, dtype=np.float64), (1, n_form)))
        dt3 = float(time_3[1] - time_3[0])
        # elapsed time: phase 1 ends per formation at its own stop row; the loop count follows the slowest formation
        stop = ph1['stop_row'].cpu().numpy()
        t_final = float((np.max(np.minimum(stop, len(ph1['time']))) - 1) * t_step + dur2)
        X_last = ph2['X_final']
        k = 0
        while t_final <= t_sim_end:
            if F is not None:
                kw2 = dict(t_start=t2d + (float(dur2) + k * float(time_3[-1])))
            ph3 = ctx.track_run(x3, y3, X_last, dt3, record=record3, **kw, **kw2, **gk(2 + k, gs, track=True))
            gs = ph3.get('gust_state')
            out['phase3'].append(ph3)
            if audit is not None:
                t3 = float(dur2) + k * float(time_3[-1])
                out['audit']['phase3'].append(ctx.flight_audit(ph3['X'], n_ac, dt3, t_start=t3 if t2a is None else t2a + t3, x_ref=x3,
                                                               y_ref=y3, **akw))
                if fleet:
                    out['audit']['phase3'][-1]['fleet'] = _fleet_audit(ctx, audit, ph3['X'], n_ac, dt3, n_form, t_start=t2)
            X_last = ph3['X_final']
            t_final += float(time_3[-1])
            k += 1
    if est is not None:
        out['wind_fit'] = dict(estimate=known, stats=known.stats, support=known.support, rms=known.rms)
    return out


def run_simulation_batch(time, Yrefs, X0s, perts=None, w=(0., 0.), record=('X', 'U', 'Xr'), windfield=None):
    """The legacy DFFFController loop for n independent aircraft.  Yrefs (T, n, >=3, 2): each trajectory's traj.get(t) at
    the sample times; X0s (n, 5); perts (T, n, 5) or None.  Device dictionary out (plane-major [T][.][n]).  windfield: a
    SplineWindField instead of w: the plant flies it and the controller samples it at the reference point (row i at time[i])."""
    fld = plant_wind(windfield)
    ctx = d2dhip.default_context()
    ac = ddyn.Aircraft()
    Y = np.asarray(Yrefs, dtype=np.float64)
    T, n = Y.shape[:2]
    Yd = np.ascontiguousarray(Y[:, :, :3, :].transpose(0, 2, 3, 1).reshape(T, 6, n))      # rows x, y, xd, yd, xdd, ydd
    dP = None if perts is None else ctx.dev(np.ascontiguousarray(np.asarray(perts, dtype=np.float64).transpose(0, 2, 1)))
    return ctx.dfff_run(ctx.dev(Yd), ctx.dev(_planes(np.asarray(X0s, dtype=np.float64))), float(time[1] - time[0]), perts=dP,
                        record=record, w=(float(w[0]), float(w[1])), tau_phi=ac.tau_phi, tau_v=ac.tau_v,
                        **({} if fld is None else dict(wind=fld, t_start=float(time[0]))))


def run_simulation(time, aircraft, windfield, ctl, X0, perts):
    """One aircraft, the reference's triple X (T,5), U (T,2), Yref (T,4,2) (src/05_test_simulation.py:21-34); ctl is a
    d2d.guidance.DFFFController (its trajectory is sampled on the host, the time loop runs on the GPU)."""
    Yref = np.array([ctl.traj.get(t) for t in time])
    fld = plant_wind(windfield)
    w = windfield.sample(time[0], Yref[0, 0]) if fld is None else (0., 0.)
    out = run_simulation_batch(time, Yref[:, None], np.asarray(X0, dtype=np.float64)[None], None if perts is None else np.asarray(perts)[:, None],
                               w=w, record=('X', 'U'), windfield=fld)
    d2dhip.default_context().sync()
    return out['X'].cpu().numpy()[:, :, 0], out['U'].cpu().numpy()[:, :, 0], Yref


def sample_references_batch(trajs, time):
    """Flat outputs of many reference trajectories at the sample times, as run_simulation_batch wants them: device tensor
    [T][6][n].  Trajectories with a descriptor (lines, circle arcs, slaloms, min-snap polynomials, composites of them:
    d2d.trajectory.describe) are evaluated by d2d_traj_sample on the GPU -- the reference calls traj.get(t) in a Python loop per
    aircraft and step (src/05_test_simulation.py:25); the others (splines, space-indexed, tabulated) are sampled on the host and
    uploaded into their columns."""
    import d2d.trajectory as ddt
    ctx = d2dhip.default_context()
    time = np.asarray(time, dtype=np.float64)
    T, n = len(time), len(trajs)
    dt = float(time[1] - time[0])
    rows = [ddt.describe(tr) for tr in trajs]
    dev_ok = [r is not None for r in rows]
    desc = np.stack([r if r is not None else np.zeros(d2dhip.TRAJ_STRIDE) for r in rows])
    Y = ctx.traj_sample(ctx.dev(desc), T, float(time[0]), dt)
    for j, tr in enumerate(trajs):
        if not dev_ok[j]:
            Yh = np.array([np.asarray(tr.get(t))[:3].reshape(-1) for t in time])       # rows x, y, xd, yd, xdd, ydd
            Y[:, :, j] = ctx.dev(np.ascontiguousarray(Yh))
    return Y


def test_simulation(scen, record=('X', 'U')):
    """src/05_test_simulation.py:37-54 without the plots: every aircraft of a d2d.scenario.Scenario flown with the DFFFController
    along its reference, all of them in ONE device loop.  Returns Xs, Us (lists of (T, 5) / (T, 2) arrays, one per aircraft)
    and Yrefs (T, n, 3, 2)."""
    ctx = d2dhip.default_context()
    time = np.asarray(scen.time, dtype=np.float64)
    n = len(scen.trajs)
    Y = sample_references_batch(scen.trajs, time)                                        # dev [T][6][n]
    ac = scen.aircrafts[0]
    fld = plant_wind(scen.windfield)
    w = scen.windfield.sample(time[0], None) if fld is None else (0., 0.)
    perts = ctx.dev(np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64) for p in scen.perts[:n]], 2)))   # [T][5][n]
    X0 = np.stack([np.asarray(x, dtype=np.float64) for x in scen.X0s[:n]])
    out = ctx.dfff_run(Y, ctx.dev(_planes(X0)), float(time[1] - time[0]), perts=perts, record=record,
                       w=(float(w[0]), float(w[1])), tau_phi=ac.tau_phi, tau_v=ac.tau_v,
                       **({} if fld is None else dict(wind=fld, t_start=float(time[0]))))
    ctx.sync()
    Xh, Uh, Yh = out['X'].cpu().numpy(), out['U'].cpu().numpy(), Y.cpu().numpy()
    Yrefs = Yh.transpose(0, 2, 1).reshape(len(time), n, 3, 2)
    return [Xh[:, :, j] for j in range(n)], [Uh[:, :, j] for j in range(n)], Yrefs
