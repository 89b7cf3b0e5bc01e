"""ctypes binding of libd2dhip.so (include/d2d.h) -- the only way host code reaches the
HIP kernels.  PyTorch-ROCm tensors are used purely as device buffers (data_ptr()) and
for the stream; no torch op takes part in the numerics.

There is no CPU fallback: importing this module without the built library raises.
"""
import ctypes as C
import os

import numpy as np

from .plan import nlp_plan       # noqa: F401  (the planners' choice among the nlp_solve* methods of a Context)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('D2D_LIB') or os.path.join(os.path.dirname(_HERE), 'lib', 'libd2dhip.so')   # D2D_LIB: A/B builds

SCEN_STRIDE = 80
MAX_OBS = 16
MAX_MOV, MOV_MAX_KNOT = 8, 32          # include/d2d.h D2D_MAX_MOV / D2D_MOV_MAX_KNOT (tests compare)
MAX_VIA = 16                           # include/d2d.h D2D_MAX_VIA
MAX_KEEP = 8                           # include/d2d.h D2D_MAX_KEEP
MAX_FENCE = 8                          # include/d2d.h D2D_MAX_FENCE
(SC_X0, SC_Y0, SC_PSI0, SC_X1, SC_Y1, SC_PSI1, SC_VREF, SC_VSP, SC_KV, SC_KPHI, SC_KOBS, SC_S,
 SC_WWP, SC_WX, SC_WY, SC_GOLEFT, SC_O0X, SC_O0Y, SC_O0R, SC_O1X, SC_O1Y, SC_O1R, SC_WBND,
 SC_PHIMAX, SC_VMIN, SC_VMAX, SC_KCOL, SC_RCOL, SC_SCOL, SC_PMASK, SC_OKIND, SC_BANKMAX, SC_OEXT) = range(33)
SC_XMIN, SC_XMAX, SC_YMIN, SC_YMAX = range(SC_OEXT + 3 * (MAX_OBS - 2), SC_OEXT + 3 * (MAX_OBS - 2) + 4)   # soft position box


def obs_col(i):
    """First of the three columns (x, y, r) of static obstacle i in a scenario row (include/d2d.h D2D_SC_OEXT)."""
    return SC_O0X + 3 * i if i < 2 else SC_OEXT + 3 * (i - 2)


TRAJ_MAX_SEG, TRAJ_SEG_STRIDE = 8, 20
TRAJ_STRIDE = 4 + TRAJ_MAX_SEG * TRAJ_SEG_STRIDE
TRAJ_LINE, TRAJ_CIRCLE, TRAJ_SLALOM, TRAJ_POLY = 1, 2, 3, 4
ST_RUNNING, ST_CONVERGED, ST_MAXITER, ST_NONFINITE, ST_STALLED = range(5)


class D2DError(RuntimeError):
    pass


class GvfParams(C.Structure):
    _fields_ = [('n_form', C.c_int32), ('n_ac', C.c_int32), ('n_rows', C.c_int32), ('rec_stride', C.c_int32),
                ('dt', C.c_double), ('tau_phi', C.c_double), ('tau_v', C.c_double),
                ('ke', C.c_double), ('kd', C.c_double), ('kr', C.c_double), ('v_c', C.c_double),
                ('wx', C.c_double), ('wy', C.c_double), ('use_stop', C.c_int32), ('stop_hold', C.c_int32),
                ('stop_tol', C.c_double * 3)]


class TrackParams(C.Structure):
    _fields_ = [('n', C.c_int32), ('n_rows', C.c_int32), ('dt', C.c_double), ('tau_phi', C.c_double),
                ('tau_v', C.c_double), ('wx', C.c_double), ('wy', C.c_double),
                ('err_sats', C.c_double * 5), ('v_min', C.c_double), ('v_max', C.c_double),
                ('phi_lim', C.c_double), ('q_diag', C.c_double * 5), ('r_diag', C.c_double * 2)]


class WindFieldC(C.Structure):
    """d2d_wind_field (include/d2d.h): a uniform tensor-product cubic B-spline wind field; cp is a device address."""
    _fields_ = [('nt', C.c_int32), ('ny', C.c_int32), ('nx', C.c_int32), ('pad', C.c_int32),
                ('t0', C.c_double), ('ht', C.c_double), ('x0', C.c_double), ('hx', C.c_double), ('y0', C.c_double), ('hy', C.c_double),
                ('cp', C.c_void_p)]


WIND_TOL, WIND_MAX_ITERS = 1e-13, 8          # include/d2d.h D2D_WIND_*


class GustC(C.Structure):
    """d2d_gust (include/d2d.h): a stochastic gust of the plant; state_in, state_out, g_hist are device addresses or None."""
    _fields_ = [('seed', C.c_uint64), ('stream_base', C.c_int64), ('phase', C.c_int32), ('n_ac', C.c_int32), ('step_base', C.c_int64),
                ('a', C.c_double), ('s', C.c_double), ('sigma', C.c_double), ('w_own', C.c_double), ('w_form', C.c_double),
                ('state_in', C.c_void_p), ('state_out', C.c_void_p), ('g_hist', C.c_void_p)]


class NlpOpts(C.Structure):
    _fields_ = [('rho0', C.c_double), ('mub0', C.c_double), ('mub_min', C.c_double), ('feas_tol', C.c_double),
                ('opt_tol', C.c_double), ('inner_max', C.c_int32), ('outer_max', C.c_int32), ('serial', C.c_int32), ('slots', C.c_int32),
                ('bounds', C.c_void_p), ('order', C.c_void_p)]


class NlpModel(C.Structure):
    """d2d_nlp_model: device pointers of the quadratic objective model (g [B][5][N], H [B][15][N] upper triangles, Wc [B][5][N])."""
    _fields_ = [('g', C.c_void_p), ('H', C.c_void_p), ('Wc', C.c_void_p)]


class MovingObstaclesC(C.Structure):
    """d2d_moving_obstacles (include/d2d.h): knots dev [G][n_mov][n_knot][3] = (t, x, y), disc dev [G][n_mov][2] = (r, kind)."""
    _fields_ = [('n_mov', C.c_int32), ('n_knot', C.c_int32), ('knots', C.c_void_p), ('disc', C.c_void_p)]


class ViaPointsC(C.Structure):
    """d2d_via_points (include/d2d.h): pts dev [G][n_via][5] = (node, mask, x, y, psi); mask bits 0..2 = x, y, psi pinned, 0 = absent."""
    _fields_ = [('n_via', C.c_int32), ('pts', C.c_void_p)]


class KeepOutC(C.Structure):
    """d2d_keep_out (include/d2d.h): discs dev [B][n_keep][3] = (cx, cy, R), a row with R <= 0 absent."""
    _fields_ = [('n_keep', C.c_int32), ('pad', C.c_int32), ('discs', C.c_void_p)]


class FenceC(C.Structure):
    """d2d_fence (include/d2d.h): edges dev [B][n_edge][4] = (ax, ay, b, kap), a row with ax = ay = 0 absent."""
    _fields_ = [('n_edge', C.c_int32), ('pad', C.c_int32), ('edges', C.c_void_p)]


class DispersionIn(C.Structure):
    """d2d_dispersion_in (include/d2d.h): the gust's a, s, sigma and S_in, a device address [28][n] or None."""
    _fields_ = [('a', C.c_double), ('s', C.c_double), ('sigma', C.c_double), ('S_in', C.c_void_p)]


DISPERSION_OUT = ('Ppos_hist', 'S_out', 'sig_max', 'sig_row', 'fence_sn', 'fence_k', 'fence_row', 'disc_k', 'disc_row')


class DispersionOut(C.Structure):
    """d2d_dispersion_out (include/d2d.h): device addresses, any may be None."""
    _fields_ = [(k, C.c_void_p) for k in DISPERSION_OUT]


class AuditParams(C.Structure):
    """d2d_audit_params (include/d2d.h)."""
    _fields_ = [('n_form', C.c_int32), ('n_ac', C.c_int32), ('n_rows', C.c_int32), ('rows_per_block', C.c_int32), ('n_stat', C.c_int32),
                ('reserved', C.c_int32), ('dt_row', C.c_double), ('d_safe', C.c_double), ('err_tol', C.c_double)]


AUDIT_OUT = ('sep_dist', 'sep_partner', 'sep_time', 'sep_count', 'stat_clear', 'stat_time', 'stat_count', 'mov_clear', 'mov_time', 'mov_count',
             'err_max', 'err_time', 'err_count', 'phi_max', 'v_min', 'v_max', 'status')
AUDIT_NONFINITE, AUDIT_BAD_TSTART, AUDIT_BAD_TRACK = 1, 2, 4     # include/d2d.h D2D_AUDIT_*: the bits of a refused formation's status


class AuditOut(C.Structure):
    """d2d_audit_out (include/d2d.h): device addresses of the outputs, None for one that is not wanted."""
    _fields_ = [(k, C.c_void_p) for k in AUDIT_OUT]


class FleetParams(C.Structure):
    """d2d_fleet_params (include/d2d.h)."""
    _fields_ = [('n_form', C.c_int32), ('n_ac', C.c_int32), ('n_rows', C.c_int32), ('g_rows', C.c_int32), ('tile_rows', C.c_int32),
                ('slots', C.c_int32), ('dt_row', C.c_double), ('d_look', C.c_double), ('step_max', C.c_double), ('d_safe', C.c_double)]


FLEET_OUT = ('near_dist', 'near_partner', 'near_time', 'near_count', 'status')
FLEET_NONFINITE, FLEET_STEP, FLEET_BAD_ROW0, FLEET_RANGE = 1, 2, 4, 8     # include/d2d.h D2D_FLEET_*: the bits of a refused formation's status


class FleetOut(C.Structure):
    """d2d_fleet_out (include/d2d.h): device addresses of the outputs, None for one that is not wanted."""
    _fields_ = [(k, C.c_void_p) for k in FLEET_OUT]


TRACKS_OUT = ('knots', 'disc', 'partner', 'part_dist', 'part_time', 'chord_err', 'n_conf', 'status')
TRACKS_SHORT = 16                                 # include/d2d.h D2D_TRACKS_SHORT: fewer valid rows than knots


class TracksOut(C.Structure):
    """d2d_tracks_out (include/d2d.h): device addresses of the outputs, None for one that is not wanted."""
    _fields_ = [(k, C.c_void_p) for k in TRACKS_OUT]


GUESS_OUT = ('status', 'word', 'v', 'rho', 'L', 't_nat')
GUESS_FIT, GUESS_SHORT, GUESS_LOOSE, GUESS_LOOSE_UNMET, GUESS_LINE, GUESS_INVALID = range(6)     # include/d2d.h D2D_GUESS_*
GUESS_STATUS = ('FIT', 'SHORT', 'LOOSE', 'LOOSE_UNMET', 'LINE', 'INVALID')
GUESS_WORDS = ('LSL', 'RSR', 'LSR', 'RSL', 'RLR', 'LRL')      # the word index of d2d_nlp_guess_dubins (-1: none)
GUESS_KAPPA = 0.9                      # include/d2d.h D2D_GUESS_KAPPA


class NlpGuessOpts(C.Structure):
    """d2d_nlp_guess_opts (include/d2d.h): bounds and v_pref are device addresses or None."""
    _fields_ = [('kappa', C.c_double), ('bounds', C.c_void_p), ('v_pref', C.c_void_p), ('waves', C.c_int32), ('reserved', C.c_int32)]


class NlpGuessOut(C.Structure):
    """d2d_nlp_guess_out (include/d2d.h): device addresses of the outputs, None for one that is not wanted."""
    _fields_ = [(k, C.c_void_p) for k in GUESS_OUT]


WINDFIT_MAX_CP, WINDFIT_CHUNK = 4096, 64     # include/d2d.h D2D_WINDFIT_*
WINDFIT_STATS = ('used', 'nonfinite', 'outside', 'over', 'rss_x', 'rss_y', 'cg_iters', 'cg_resid')   # the eight numbers of stats


class WindFitParams(C.Structure):
    """d2d_windfit_params (include/d2d.h)."""
    _fields_ = [('n_form', C.c_int32), ('n_ac', C.c_int32), ('n_rows', C.c_int32), ('cg_max', C.c_int32), ('waves', C.c_int32),
                ('reserved', C.c_int32), ('dt_row', C.c_double), ('w_max', C.c_double), ('lam_x', C.c_double), ('lam_y', C.c_double),
                ('lam_t', C.c_double), ('mu', C.c_double), ('cg_tol', C.c_double)]


class WindFitOut(C.Structure):
    """d2d_windfit_out (include/d2d.h): device addresses of the optional outputs, None for one that is not wanted."""
    _fields_ = [(k, C.c_void_p) for k in ('support', 'stats', 'H_out', 'b_out')]


class FitOpts(C.Structure):
    _fields_ = [('max_iter', C.c_int32), ('check_every', C.c_int32), ('ftol', C.c_double),
                ('gtol', C.c_double), ('xtol', C.c_double), ('so_lambda', C.c_double),
                ('mode', C.c_int32), ('mp_finish', C.c_int32), ('mp_ftol', C.c_double), ('mp_xtol', C.c_double),
                ('mp_gtol', C.c_double), ('slice', C.c_int32), ('mp_slow', C.c_int32),
                ('handout', C.c_int32), ('prio_at', C.c_int32), ('gs_ls', C.c_int32), ('gs_ls_s0', C.c_int32), ('gs_ls_r0', C.c_double),
                ('gs_prio_at', C.c_int32), ('gs_pairs', C.c_int32)]


class FitPlanOpts(C.Structure):
    _fields_ = [('kernel', C.c_int32), ('long_tables', C.c_int32), ('reserved', C.c_int32 * 2)]


SO_LAMBDA = 1e-4          # D2D_LM_SO_LAMBDA: damping below which the evaluations carry the second-order term (FAST mode)
NLP_INNER_MAX, NLP_OUTER_MAX = 20, 120     # include/d2d.h D2D_NLP_INNER_MAX / D2D_NLP_OUTER_MAX (tests/test_abi.py compares)
MODE_MINPACK, MODE_FAST = 0, 1     # D2D_LM_MODE_*: MINPACK's lmder path (what scipy least_squares('lm') follows) / rounds 1-2's loop
MP_FINISH = 3             # D2D_LM_MP_FINISH: calm lmder steps before the second-order finish (0 = pure lmder)
MP_SLOW = 8               # D2D_LM_MP_SLOW: stagnating lmder trials (cost change <= 1e-4 of itself) in a row before the finish (0 = never)
SLICE = 0                 # D2D_LM_SLICE: iterations a fit runs before it yields its wavefront to waiting fits (0 = never)
HANDOUT_INDEX, HANDOUT_PREDICTED = 0, 1   # D2D_HANDOUT_*: hand-out order of a batch larger than the resident wavefronts
PRIO_AT = 48              # D2D_LM_PRIO_AT
GS_LS_SWEEP0, GS_LS_RATIO, GS_PRIO_AT = 8, 0.8, 40     # D2D_GS_LS_SWEEP0 / D2D_GS_LS_RATIO / D2D_GS_PRIO_AT
KERNEL_AUTO, KERNEL_SPLIT, KERNEL_FUSED, KERNEL_LONG, KERNEL_KNOT = -1, 0, 1, 2, 3     # D2D_FIT_KERNEL_*
KERNELS = {'auto': KERNEL_AUTO, 'split': KERNEL_SPLIT, 'fused': KERNEL_FUSED, 'long': KERNEL_LONG, 'knot': KERNEL_KNOT}


def fit_opts(max_iter=200, check_every=8, ftol=1e-14, gtol=1e-9, xtol=1e-11, so_lambda=SO_LAMBDA, mode=MODE_MINPACK,
             mp_finish=MP_FINISH, mp_tol=1e-15, slice=SLICE, mp_slow=MP_SLOW, handout=HANDOUT_PREDICTED, prio_at=PRIO_AT,
             gs_ls=1, gs_ls_s0=GS_LS_SWEEP0, gs_ls_r0=GS_LS_RATIO, gs_prio_at=GS_PRIO_AT, gs_pairs=0):
    """d2d_fit_opts with the library's defaults (include/d2d.h; tests/test_abi.py compares them with d2d_fit_opts_default)."""
    return FitOpts(max_iter, check_every, ftol, gtol, xtol, so_lambda, mode, mp_finish, mp_tol, mp_tol, mp_tol, slice, mp_slow,
                   handout, prio_at, gs_ls, gs_ls_s0, gs_ls_r0, gs_prio_at, gs_pairs)


_P = C.c_void_p
_SIGS = {
    'd2d_version': (C.c_int, []),
    'd2d_last_error': (C.c_char_p, []),
    'd2d_ctx_create': (C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    'd2d_ctx_destroy': (C.c_int, [_P]),
    'd2d_ctx_sync': (C.c_int, [_P]),
    'd2d_comm_available': (C.c_int, []),
    'd2d_comm_unique_id': (C.c_int, [_P]),
    'd2d_comm_create': (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    'd2d_comm_destroy': (C.c_int, [_P]),
    'd2d_comm_info': (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'd2d_allreduce_stats': (C.c_int, [_P, _P, _P]),
    'd2d_step': (C.c_int, [_P, C.c_int, _P, _P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P]),
    'd2d_sim_gvf_run': (C.c_int, [_P, C.POINTER(GvfParams)] + [_P] * 13),
    'd2d_ctrl_gain': (C.c_int, [_P, C.POINTER(TrackParams)] + [_P] * 6),
    'd2d_dfff_eval': (C.c_int, [_P, C.POINTER(TrackParams)] + [_P] * 5),
    'd2d_sim_dfff_run': (C.c_int, [_P, C.POINTER(TrackParams)] + [_P] * 7),
    'd2d_sim_track_run': (C.c_int, [_P, C.POINTER(TrackParams)] + [_P] * 10),
    'd2d_wind_sample': (C.c_int, [_P, C.POINTER(WindFieldC), C.c_int, _P, _P, _P]),
    'd2d_step_wind': (C.c_int, [_P, C.c_int, _P, _P, C.c_double, C.POINTER(WindFieldC), C.c_double, C.c_double, C.c_double, _P, _P]),
    'd2d_sim_gvf_run_wind': (C.c_int, [_P, C.POINTER(GvfParams)] + [_P] * 13 + [C.POINTER(WindFieldC), C.c_double, _P]),
    'd2d_sim_track_run_wind': (C.c_int, [_P, C.POINTER(TrackParams)] + [_P] * 10 + [C.POINTER(WindFieldC), C.c_double, _P]),
    'd2d_sim_dfff_run_wind': (C.c_int, [_P, C.POINTER(TrackParams)] + [_P] * 7 + [C.POINTER(WindFieldC), C.c_double, _P]),
    'd2d_sim_track_run_wind_at': (C.c_int, [_P, C.POINTER(TrackParams)] + [_P] * 10 + [C.POINTER(WindFieldC), _P, _P]),
    'd2d_gust_sample': (C.c_int, [_P, C.c_int64, C.c_int, C.POINTER(GustC)]),
    'd2d_sim_gvf_run_gust': (C.c_int, [_P, C.POINTER(GvfParams)] + [_P] * 13 + [C.POINTER(WindFieldC), C.c_double, _P, C.POINTER(GustC)]),
    'd2d_sim_track_run_gust': (C.c_int, [_P, C.POINTER(TrackParams)] + [_P] * 10 + [C.POINTER(WindFieldC), _P, _P, C.POINTER(GustC)]),
    'd2d_traj_sample': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, C.c_double, _P, _P]),
    'd2d_dcf_eval': (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_double, _P, _P, _P, _P]),
    'd2d_gvf_eval': (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_double, C.c_double, _P]),
    'd2d_flatness': (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P, _P]),
    'd2d_cont_jac': (C.c_int, [_P, C.c_int, _P, C.c_double, C.c_double, _P, _P]),
    'd2d_lqr': (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    'd2d_nlp_workspace_doubles': (C.c_int, [C.c_int]),
    'd2d_nlp_solve': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 8),
    'd2d_nlp_solve_wind': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 7 + [C.POINTER(WindFieldC), C.c_double]),
    'd2d_nlp_free_workspace_doubles': (C.c_int, [C.c_int]),
    'd2d_nlp_solve_free': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 9),
    'd2d_nlp_solve_groups': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts), C.c_int, C.c_double] + [_P] * 9),
    'd2d_nlp_solve_groups_wind': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts), C.c_int, C.c_double] + [_P] * 9
                                  + [C.POINTER(WindFieldC), _P]),
    'd2d_nlp_solve_groups_pairs': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts), C.c_int, C.c_double] + [_P] * 9
                                   + [C.POINTER(WindFieldC), _P]),
    'd2d_nlp_solve_model': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts), C.POINTER(NlpModel)] + [_P] * 7),
    'd2d_mov_sample': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(MovingObstaclesC), _P]),
    'd2d_nlp_solve_moving': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 7
                             + [C.POINTER(WindFieldC), _P, C.POINTER(MovingObstaclesC), _P]),
    'd2d_nlp_solve_groups_moving': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts), C.c_int, C.c_double] + [_P] * 9
                                    + [C.POINTER(WindFieldC), _P, C.POINTER(MovingObstaclesC), _P]),
    'd2d_nlp_solve_keepout': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 7
                              + [C.POINTER(WindFieldC), _P, C.POINTER(KeepOutC), _P]),
    'd2d_nlp_solve_fence': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 7
                            + [C.POINTER(WindFieldC), _P, C.POINTER(KeepOutC), _P, C.POINTER(FenceC), _P]),
    'd2d_nlp_solve_free_fence': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 9
                                 + [C.POINTER(KeepOutC), _P, C.POINTER(FenceC), _P]),
    'd2d_nlp_solve_groups_fence': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts), C.c_int, C.c_double] + [_P] * 9
                                   + [C.POINTER(WindFieldC), _P, C.POINTER(FenceC), _P]),
    'd2d_nlp_solve_keepout_moving': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 7
                                     + [C.POINTER(WindFieldC), _P, C.POINTER(MovingObstaclesC), _P, _P]),
    'd2d_nlp_solve_groups_keepout': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts), C.c_int, C.c_double] + [_P] * 9
                                     + [C.POINTER(WindFieldC), _P, C.POINTER(MovingObstaclesC), _P, _P]),
    'd2d_nlp_solve_via': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts)] + [_P] * 7
                          + [C.POINTER(WindFieldC), _P, C.POINTER(MovingObstaclesC), _P, C.POINTER(ViaPointsC), _P]),
    'd2d_nlp_solve_groups_via': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpOpts), C.c_int, C.c_double] + [_P] * 9
                                 + [C.POINTER(WindFieldC), _P, C.POINTER(MovingObstaclesC), _P, C.POINTER(ViaPointsC), _P]),
    'd2d_flight_audit_workspace': (C.c_int64, [C.POINTER(AuditParams), C.c_int]),
    'd2d_flight_audit': (C.c_int, [_P, C.POINTER(AuditParams)] + [_P] * 6 + [C.POINTER(MovingObstaclesC), _P, _P, C.POINTER(AuditOut)]),
    'd2d_fit_plan_create': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(_P)]),
    'd2d_fit_plan_create_ex': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(FitPlanOpts), C.POINTER(_P)]),
    'd2d_fit_opts_default': (C.c_int, [C.POINTER(FitOpts)]),
    'd2d_fit_plan_destroy': (C.c_int, [_P]),
    'd2d_fit_plan_get': (C.c_int, [_P] * 6),
    'd2d_fit_plan_kernel': (C.c_int, [_P]),
    'd2d_fit_knot_segments': (C.c_int, [C.c_int, C.c_int, C.c_double, _P, _P, _P, _P]),
    'd2d_fit_init': (C.c_int, [_P, _P, C.c_int, _P, _P]),
    'd2d_fit_project': (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    'd2d_fit_eval': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P]),
    'd2d_fit_rows': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P]),
    'd2d_fit_jtj': (C.c_int, [_P, _P, C.c_int, _P]),
    'd2d_fit_solve': (C.c_int, [_P, _P, C.c_int, _P, _P, C.POINTER(FitOpts), _P, _P, _P, _P]),
    'd2d_fit_begin': (C.c_int, [_P, _P, C.c_int]),
    'd2d_fit_iterate': (C.c_int, [_P, _P, C.c_int, _P, _P, C.POINTER(FitOpts), C.c_int, C.POINTER(C.c_int32)]),
    'd2d_fit_finish': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, _P, _P]),
    'd2d_fit_plan_set_order': (C.c_int, [_P, _P, C.c_int, _P]),
    'd2d_fit_plan_set_handout_prior': (C.c_int, [_P, _P, _P]),
    'd2d_fit_plan_get_order': (C.c_int, [_P, _P, C.c_int, _P]),
    'd2d_fit_plan_set_group_order': (C.c_int, [_P, _P, C.c_int, C.c_int]),
    'd2d_fit_group_report': (C.c_int, [_P, _P, C.c_int, _P, _P]),
    'd2d_fit_plan_set_groups': (C.c_int, [_P, C.c_int]),
    'd2d_fit_solve_groups': (C.c_int, [_P, _P, C.c_int, _P, _P, C.POINTER(FitOpts), C.c_int, C.c_int, C.c_double, _P,
                                       C.POINTER(C.c_int32), _P]),
    'd2d_fit_profile': (C.c_int, [_P, C.c_int]),
    'd2d_fit_profile_read': (C.c_int, [_P, _P]),
    'd2d_fit_coeffs': (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    'd2d_fit_sample': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P]),
    'd2d_nlp_guess_dubins': (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _P, C.POINTER(NlpGuessOpts), _P, C.POINTER(NlpGuessOut)]),
    'd2d_fleet_audit_workspace': (C.c_int64, [C.POINTER(FleetParams)]),
    'd2d_fleet_audit': (C.c_int, [_P, C.POINTER(FleetParams), _P, _P, _P, _P, _P, C.POINTER(FleetOut)]),
    'd2d_fleet_tracks_workspace': (C.c_int64, [C.POINTER(FleetParams), C.c_int]),
    'd2d_fleet_tracks': (C.c_int, [_P, C.POINTER(FleetParams), _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, _P,
                                   C.POINTER(TracksOut)]),
    'd2d_wind_fit_workspace': (C.c_int64, [C.POINTER(WindFitParams), C.POINTER(WindFieldC)]),
    'd2d_wind_fit': (C.c_int, [_P, C.POINTER(WindFitParams), _P, _P, _P, C.POINTER(WindFieldC), _P, _P, C.POINTER(WindFitOut)]),
    'd2d_track_dispersion': (C.c_int, [_P, C.POINTER(TrackParams), _P, _P, C.POINTER(DispersionIn), C.POINTER(FenceC), C.POINTER(KeepOutC),
                                       C.POINTER(DispersionOut)]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def load():
    """dlopen libd2dhip.so and declare every signature; fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise D2DError(f'{LIB_PATH} not found: build it with __graft_entry__.build() '
                       f'(make -C drone-sim-python_amd/csrc); there is no CPU fallback')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise D2DError(f'libd2dhip error {rc}: {load().d2d_last_error().decode()}')


def knot_segments(S, K, duration):
    """(host, no GPU) sample geometry of a knot-coordinate plan: (k0 [S+1], seg_min, seg_max, seg_floor) -- d2d_fit_knot_segments."""
    import numpy as np
    k0 = np.zeros(S + 1, dtype=np.int32)
    out = (C.c_int32 * 3)()
    p = [C.cast(C.byref(out, 4 * i), C.c_void_p) for i in range(3)]
    _check(load().d2d_fit_knot_segments(S, K, float(duration), _hptr(k0), *p))
    return k0, int(out[0]), int(out[1]), int(out[2])


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise D2DError('no HIP device visible to PyTorch-ROCm; the d2d engine has no CPU fallback')
    return torch


_ABSENT = object()      # an optional input that an entry point does not take (None is a value: no field, nothing moves, no pins)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _hptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _wind_c(ctx, wind):
    """A d2d_wind_field for `wind`: a WindFieldC (whose cp the caller keeps alive) or an object with device_field(ctx) -> WindFieldC
    (d2d.wind.SplineWindField: its device copy is cached per context)."""
    if isinstance(wind, WindFieldC):
        return wind
    if hasattr(wind, 'device_field'):
        return wind.device_field(ctx)
    raise TypeError(f'{type(wind).__name__} is not a device wind field: build one with d2d.wind.SplineWindField')


class Comm:
    """d2d_comm: the RCCL communicator of the sharded solve's convergence exchange (d2d_allreduce_stats)."""

    def __init__(self, ctx, uid, rank, world):
        assert len(uid) == 128
        self.ctx = ctx
        h = _P()
        _check(ctx.lib.d2d_comm_create(ctx.h, C.c_char_p(uid), int(rank), int(world), C.byref(h)))
        self.h = h

    def info(self):
        r, w = C.c_int32(-1), C.c_int32(-1)
        _check(self.ctx.lib.d2d_comm_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def allreduce_stats(self, stats_dev):
        """stats_dev: device tensor of three doubles, in place: [0] sum, [1] max, [2] sum over the ranks; enqueued on the context's stream."""
        assert stats_dev.is_cuda and stats_dev.dtype == _torch().float64 and stats_dev.numel() == 3 and stats_dev.is_contiguous()
        _check(self.ctx.lib.d2d_allreduce_stats(self.ctx.h, self.h, _ptr(stats_dev)))

    def close(self):
        if getattr(self, 'h', None):
            self.ctx.lib.d2d_comm_destroy(self.h)
            self.h = None

    __del__ = close


class Context:
    """d2d_ctx bound to the current torch stream of `device`."""

    def __init__(self, device=0):
        torch = _torch()
        self.lib = load()
        self.device = torch.device('cuda', device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.current_stream(self.device)
        h = _P()
        _check(self.lib.d2d_ctx_create(device, C.c_void_p(self.stream.cuda_stream), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.d2d_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def sync(self):
        _check(self.lib.d2d_ctx_sync(self.h))

    # -- multi-GPU convergence exchange through the C-ABI (RCCL, include/d2d.h d2d_comm_*) ------------
    def comm_available(self):
        """local, no communication: can this process load RCCL (d2d_comm_available)?  None when it can, else the reason."""
        rc = self.lib.d2d_comm_available()
        return None if rc == 0 else self.lib.d2d_last_error().decode()

    def comm_unique_id(self):
        """128 opaque bytes (ncclGetUniqueId): rank 0 creates them, the host hands them to the other ranks."""
        buf = C.create_string_buffer(128)
        _check(self.lib.d2d_comm_unique_id(buf))
        return buf.raw

    def comm_create(self, uid, rank, world):
        """d2d_comm of this context's device (ncclCommInitRank): every rank, same uid."""
        return Comm(self, uid, rank, world)

    # -- buffers --------------------------------------------------------------------
    def dev(self, a, dtype=None):
        """numpy array (or tensor) -> contiguous device tensor."""
        torch = _torch()
        if isinstance(a, torch.Tensor):
            t = a.to(self.device)
        else:
            t = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        if dtype is not None:
            t = t.to(dtype)
        return t.contiguous()

    def empty(self, *shape, dtype=None):
        torch = _torch()
        return torch.empty(*shape, dtype=dtype or torch.float64, device=self.device)

    def zeros(self, *shape, dtype=None):
        torch = _torch()
        return torch.zeros(*shape, dtype=dtype or torch.float64, device=self.device)

    # -- plant / guidance -----------------------------------------------------------
    def step(self, X, U, W=(0.0, 0.0), tau_phi=0.01, tau_v=1.0, dt=0.05):
        """X dev [5][n], U dev [2][n] -> Xnext dev [5][n]   (Aircraft.disc_dyn, batched)."""
        n = X.shape[1]
        out = self.empty(5, n)
        _check(self.lib.d2d_step(self.h, n, _ptr(X), _ptr(U), W[0], W[1], tau_phi, tau_v, dt, _ptr(out)))
        return out

    def wind_sample(self, wind, t, xy):
        """d2d_wind_sample: the field at t dev [n], xy dev [2][n] -> w dev [2][n] (wx, wy)."""
        n = t.shape[0]
        assert t.is_contiguous() and xy.is_contiguous() and tuple(xy.shape) == (2, n)
        w = self.empty(2, n)
        f = _wind_c(self, wind)
        _check(self.lib.d2d_wind_sample(self.h, C.byref(f), n, _ptr(t), _ptr(xy), _ptr(w)))
        return w

    def step_wind(self, X, U, t, wind, tau_phi=0.01, tau_v=1.0, dt=0.05, iter_max=None):
        """X dev [5][n], U dev [2][n], the step's start time t, a field -> Xnext dev [5][n] (Aircraft.disc_dyn in a field, batched).
        iter_max: dev int32 [1] that receives the largest fixed-point sweep count, or None."""
        n = X.shape[1]
        out = self.empty(5, n)
        f = _wind_c(self, wind)
        _check(self.lib.d2d_step_wind(self.h, n, _ptr(X), _ptr(U), float(t), C.byref(f), tau_phi, tau_v, dt, _ptr(out), _ptr(iter_max)))
        return out

    def _gust_c(self, gust, dt, n_ac, N, phase, state, stream_base=0, step_base=0):
        """The d2d_gust of `gust` -- a GustC (a COPY of it, state_in included: the caller's struct is not written; its state_out and
        g_hist are replaced by the method's own outputs) or a model with lower(dt, n_ac, phase, stream_base) (d2d.wind.GustModel) --
        for N drones, from `state` (dev [4][N] or None: the stationary start)."""
        if isinstance(gust, GustC):
            return GustC.from_buffer_copy(gust)
        if not hasattr(gust, 'lower'):
            raise TypeError(f'{type(gust).__name__} is not a gust model: build one with d2d.wind.GustModel')
        assert state is None or (state.is_contiguous() and tuple(state.shape) == (4, N) and state.dtype == _torch().float64 and state.device.type == 'cuda')
        g = gust.lower(float(dt), int(n_ac), int(phase), int(stream_base), int(step_base))
        g.state_in = None if state is None else state.data_ptr()
        return g

    def _plant_extras(self, out, N, n_rec, record, wind, gust=None, gust_kw=(), t_start=None):
        """The plant's optional inputs as gvf_run, track_run and dfff_run share them -> (f, t_at, g), each None when absent.  g: the GustC
        of `gust` (_gust_c with gust_kw = (dt, n_ac, phase, state, stream_base)) writing out['gust_state'] [4][N] and, with 'g' in record,
        out['g'] [n_rec][2][N]; f: the WindFieldC of `wind`, with out['iter_max']; both outputs are made unless `out` brought them.
        t_at: track_run's t_start when it is a device tensor [N], one start time per drone (that needs a field); None for a float."""
        g = None
        if gust is not None:
            g = self._gust_c(gust, *gust_kw[:2], N, *gust_kw[2:])
            if out.get('gust_state') is None:
                out['gust_state'] = self.empty(4, N)
            if 'g' in record and out.get('g') is None:
                out['g'] = self.zeros(n_rec, 2, N)
            g.state_out, g.g_hist = out['gust_state'].data_ptr(), None if out.get('g') is None else out['g'].data_ptr()
        f = None if wind is None else _wind_c(self, wind)
        if f is not None and out.get('iter_max') is None:
            out['iter_max'] = self.zeros(1, dtype=_torch().int32)
        t_at = t_start if hasattr(t_start, 'data_ptr') else None
        assert t_at is None or f is not None, 'per-drone start times (a tensor) need a wind field: without one the time is not read'
        assert t_at is None or (t_at.is_contiguous() and tuple(t_at.shape) == (N,) and t_at.dtype == _torch().float64 and t_at.device == self.device)
        return f, t_at, g

    def gust_sample(self, gust, N, n_rows, dt, n_ac=1, phase=0, state=None, stream_base=0, step_base=0, record=True):
        """The gust process alone (d2d_gust_sample): gust a d2d.wind.GustModel, N drones in formations of n_ac, rows 0 .. n_rows - 1
        at spacing dt.  state dev [4][N]: the state of row 0 (None: the stationary start); stream_base: the global index of drone 0;
        step_base: the steps a continued series has already made.  Returns dict(g dev [n_rows][2][N] (record), gust_state dev [4][N])."""
        g = self._gust_c(gust, dt, n_ac, N, phase, state, stream_base, step_base)
        out = dict(g=self.empty(n_rows, 2, N) if record else None, gust_state=self.empty(4, N))
        g.state_out, g.g_hist = out['gust_state'].data_ptr(), None if out['g'] is None else out['g'].data_ptr()
        _check(self.lib.d2d_gust_sample(self.h, int(N), int(n_rows), C.byref(g)))
        return out

    def gvf_run(self, X0, centres, radius, n_ac, n_rows, dt, v_c, ke=4e-4, kd=25.0, kr=20.0,
                B=None, z_des=None, tau_phi=0.01, tau_v=1.0, W=(0.0, 0.0), X0f=None,
                stop_tol=(3.0, 3.0, np.deg2rad(0.5)), rec_stride=1, record=('X', 'U', 'Rr', 'eth'), out=None,
                etheta_tol_deg=None, stop_hold=0, wind=None, t_start=0.0, gust=None, gust_state=None, gust_phase=0, gust_stream_base=0):
        """Circular-formation phase for N = n_form*n_ac drones.  X0 dev [5][N], centres dev
        [2][N], radius dev [N].  Returns dict of device tensors (plane-major).  out: the dictionary of an earlier
        call with the same shapes and `record` -- its buffers are written again instead of allocating new ones
        (without the stop rule every recorded row is rewritten; with it, rows behind the stop row keep their old
        content).  wind: a field the plant flies instead of W (d2d_sim_gvf_run_wind; row i at t_start + i dt); out['iter_max'] then
        holds the largest fixed-point sweep count.  gust: a d2d.wind.GustModel the plant flies on top of W or the field
        (d2d_sim_gvf_run_gust, the general kernel for every n_ac; gust_state dev [4][N]: the state of row 0, None: the stationary
        start; gust_phase: the loop's phase word; gust_stream_base: the global index of drone 0); out['gust_state'] dev [4][N] is the
        state after each formation's last executed step and, with 'g' in record, out['g'] dev [n_rec][2][N] the gust of every kept
        row.  gust None: nothing new is launched."""
        torch = _torch()
        N = X0.shape[1]
        assert N % n_ac == 0
        n_form = N // n_ac
        if B is None:
            B = np.zeros((n_ac, max(n_ac - 1, 0)))
            for i in range(n_ac - 1):
                B[i, i] = -1.0; B[i + 1, i] = 1.0
        B = np.ascontiguousarray(B, dtype=np.float64)
        z_des = np.zeros(max(n_ac - 1, 0)) if z_des is None else np.ascontiguousarray(z_des, dtype=np.float64).reshape(-1)
        # stop rule: X0f -> the state rule of case 1; etheta_tol_deg -> the phase-error rule of cases 2 / 3 (+ stop_hold steps)
        use_stop = 2 if etheta_tol_deg is not None else (1 if X0f is not None else 0)
        if use_stop == 2:
            stop_tol = (float(etheta_tol_deg), 0.0, 0.0)
        p = GvfParams(n_form, n_ac, n_rows, rec_stride, dt, tau_phi, tau_v, ke, kd, kr, v_c, W[0], W[1],
                      use_stop, int(stop_hold), (C.c_double * 3)(*stop_tol))
        n_rec = (n_rows + rec_stride - 1) // rec_stride
        if out is None:
            out = {}
            out['X'] = self.zeros(n_rec, 5, N) if 'X' in record else None
            out['U'] = self.zeros(n_rec, 2, N) if 'U' in record else None
            out['Rr'] = self.zeros(n_rec, N) if 'Rr' in record else None
            out['eth'] = self.zeros(n_rec, n_form * max(n_ac - 1, 0)) if ('eth' in record and n_ac > 1) else None
            out['X_final'] = self.empty(5, N)
            out['stop_row'] = torch.empty(n_form, dtype=torch.int32, device=self.device)
            out['conv_row'] = torch.empty(n_form, dtype=torch.int32, device=self.device)
        else:
            assert out['X_final'].shape == (5, N) and all(out[k] is None or out[k].shape[0] == n_rec for k in ('X', 'U', 'Rr', 'eth'))
        args = (self.h, C.byref(p), _ptr(X0), _ptr(centres), _ptr(radius), _hptr(B), _hptr(z_des), _ptr(X0f if use_stop == 1 else None),
                _ptr(out['X']), _ptr(out['U']), _ptr(out['Rr']), _ptr(out['eth']), _ptr(out['X_final']), _ptr(out['stop_row']),
                _ptr(out.get('conv_row')))
        f, _, g = self._plant_extras(out, N, n_rec, record, wind, gust, (dt, n_ac, gust_phase, gust_state, gust_stream_base))
        if g is not None:
            _check(self.lib.d2d_sim_gvf_run_gust(*args, None if f is None else C.byref(f), float(t_start), _ptr(out.get('iter_max')), C.byref(g)))
        elif f is None:
            _check(self.lib.d2d_sim_gvf_run(*args))
        else:
            _check(self.lib.d2d_sim_gvf_run_wind(*args, C.byref(f), float(t_start), _ptr(out['iter_max'])))
        return out

    # -- single evaluations behind the reference's per-call helpers --------------------
    def dcf_eval(self, centres, pos, n_ac, B, z_des, kr):
        """centres, pos dev [2][N] -> U_r dev [N], e_theta_deg dev [n_form*(n_ac-1)]."""
        N = pos.shape[1]; n_form = N // n_ac
        B = np.ascontiguousarray(B, dtype=np.float64); z = np.ascontiguousarray(z_des, dtype=np.float64).reshape(-1)
        Ur = self.empty(N); eth = self.empty(max(n_form * (n_ac - 1), 1))
        _check(self.lib.d2d_dcf_eval(self.h, n_form, n_ac, _hptr(B), _hptr(z), kr, _ptr(centres), _ptr(pos), _ptr(Ur), _ptr(eth)))
        return Ur, eth

    def gvf_eval(self, X, e, nvec, H, ke, kd):
        """X dev [5][n], e dev [n], nvec dev [2][n], H dev [4][n] -> dev [3][n] = U, U1, U2."""
        n = X.shape[1]
        U = self.empty(3, n)
        _check(self.lib.d2d_gvf_eval(self.h, n, _ptr(X), _ptr(e), _ptr(nvec), _ptr(H), ke, kd, _ptr(U)))
        return U

    def flatness(self, variant, Yref, W=(0.0, 0.0), tau_phi=0.01, tau_v=1.0):
        """Yref dev [8][n] -> X [5][n], U [2][n], Xdot [5][n]."""
        n = Yref.shape[1]
        X, U, Xd = self.empty(5, n), self.empty(2, n), self.empty(5, n)
        _check(self.lib.d2d_flatness(self.h, variant, n, _ptr(Yref), W[0], W[1], tau_phi, tau_v, _ptr(X), _ptr(U), _ptr(Xd)))
        return X, U, Xd

    def cont_jac(self, Xr, tau_phi=0.01, tau_v=1.0):
        n = Xr.shape[1]
        A, B = self.empty(25, n), self.empty(10, n)
        _check(self.lib.d2d_cont_jac(self.h, n, _ptr(Xr), tau_phi, tau_v, _ptr(A), _ptr(B)))
        return A, B

    def lqr(self, A, B, Q, R):
        """A dev [25][n], B dev [10][n]; Q (5,5), R (2,2) host -> K dev [10][n], P dev [25][n]."""
        n = A.shape[1]
        Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(25); R = np.ascontiguousarray(R, dtype=np.float64).reshape(4)
        K, P = self.empty(10, n), self.empty(25, n)
        _check(self.lib.d2d_lqr(self.h, n, _ptr(A), _ptr(B), _hptr(Q), _hptr(R), _ptr(K), _ptr(P)))
        return K, P

    @staticmethod
    def track_params(n, n_rows, dt, w=(0.0, 0.0), tau_phi=0.01, tau_v=1.0,
                     err_sats=(20, 20, np.pi / 3, np.pi / 4, 1), v_min=4.0, v_max=20.0,
                     phi_lim=np.deg2rad(60), Q=(1, 1, 0.1, 0.01, 0.01), R=(8, 1)):
        return TrackParams(n, n_rows, dt, tau_phi, tau_v, w[0], w[1], (C.c_double * 5)(*err_sats), v_min, v_max,
                           phi_lim, (C.c_double * 5)(*Q), (C.c_double * 2)(*R))

    def ctrl_gain(self, X, Yref, **kw):
        """X dev [5][n], Yref dev [8][n] -> Xr [5][n], dX [5][n], U [2][n], K [10][n]."""
        n = X.shape[1]
        p = self.track_params(n, 1, kw.pop('dt', 0.05), **kw)
        Xr, dX, U, K = self.empty(5, n), self.empty(5, n), self.empty(2, n), self.empty(10, n)
        _check(self.lib.d2d_ctrl_gain(self.h, C.byref(p), _ptr(X), _ptr(Yref), _ptr(Xr), _ptr(dX), _ptr(U), _ptr(K)))
        return Xr, dX, U, K

    def dfff_eval(self, X, Yref, w=(0.0, 0.0), tau_phi=0.01, tau_v=1.0):
        """DFFFController.get for n (state, reference sample) pairs: X dev [5][n], Yref dev [6][n]
        (x,y,xd,yd,xdd,ydd) -> Xr [5][n], U [2][n], K1 [6][n] (row-major 2x3)."""
        n = X.shape[1]
        p = self.track_params(n, 1, 0.01, w=w, tau_phi=tau_phi, tau_v=tau_v, phi_lim=np.deg2rad(45),
                              Q=(1, 1, 0.1, 0.0, 0.0), R=(8, 1))          # src/d2d/guidance.py:79,86
        Xr, U, K = self.empty(5, n), self.empty(2, n), self.empty(6, n)
        _check(self.lib.d2d_dfff_eval(self.h, C.byref(p), _ptr(X), _ptr(Yref), _ptr(Xr), _ptr(U), _ptr(K)))
        return Xr, U, K

    def traj_sample(self, desc, T, t_start, dt):
        """desc dev [n][TRAJ_STRIDE] trajectory descriptors (d2d.trajectory.describe) -> Yref dev [T][6][n]."""
        n = desc.shape[0]
        Y = self.empty(T, 6, n)
        _check(self.lib.d2d_traj_sample(self.h, n, T, float(t_start), float(dt), _ptr(desc), _ptr(Y)))
        return Y

    def dfff_run(self, Yref, X0, dt, perts=None, record=('X', 'U', 'Xr'), w=(0.0, 0.0), tau_phi=0.01, tau_v=1.0, out=None, wind=None,
                 t_start=0.0):
        """run_simulation of src/05_test_simulation.py with the legacy DFFFController for n aircraft: Yref dev [T][6][n]
        (x,y,xd,yd,xdd,ydd at the sample times), X0 dev [5][n], perts dev [T][5][n] or None -> dict of device histories
        X [T][5][n], U [T][2][n], Xr [T][5][n] and X_final.  wind: a field instead of w (d2d_sim_dfff_run_wind: the plant flies it, the
        controller samples it at the reference point; row i at t_start + i dt); out['iter_max']: the largest fixed-point sweep count."""
        T, _, n = Yref.shape
        p = self.track_params(n, T, dt, w=w, tau_phi=tau_phi, tau_v=tau_v, phi_lim=np.deg2rad(45),
                              Q=(1, 1, 0.1, 0.0, 0.0), R=(8, 1))          # src/d2d/guidance.py:79,86
        if out is None:
            out = {k: (self.zeros(T, c, n) if k in record else None) for k, c in (('X', 5), ('U', 2), ('Xr', 5))}
            out['X_final'] = self.empty(5, n)
        args = (self.h, C.byref(p), _ptr(Yref), _ptr(perts), _ptr(X0), _ptr(out['X']), _ptr(out['U']), _ptr(out['Xr']), _ptr(out['X_final']))
        f, _, _ = self._plant_extras(out, n, T, record, wind)
        if f is None:
            _check(self.lib.d2d_sim_dfff_run(*args))
        else:
            _check(self.lib.d2d_sim_dfff_run_wind(*args, C.byref(f), float(t_start), _ptr(out['iter_max'])))
        return out

    def _nlp_core(self, entry, scen, W, h, opts, bounds, n_ac=None, sweeps=None, want_mult=False, slots=0, order=None, mid=(),
                  field=_ABSENT, t_start=None, t_scalar=False, moving=_ABSENT, via=_ABSENT, free_rows=None, keep=_ABSENT,
                  hard_moving=False, fence=_ABSENT):
        """What the nlp_solve* methods share: the shape checks, the workspace and the outputs, d2d_nlp_opts from opts = (rho0, mub0,
        mub_min, feas_tol, opt_tol, inner_max, outer_max, serial), the call of `entry` and the result.  n_ac: a group entry (sweeps =
        (max_sweeps, tol)), R = B / n_ac scenarios with one start time and one set of tracks each; else B problems.  mid: arguments
        between W and work.  field, moving = (knots, disc), via: the optional inputs in the entries' order, _ABSENT where the entry takes
        none (it takes t_start with the field: a device array, or with t_scalar a float); each adds its entries to the result.
        free_rows: the entry is d2d_nlp_solve_free -- the rows go in front of W, the solved steps `h` [B] behind status, and the
        workspace is the larger one.  keep: the entry is d2d_nlp_solve_keepout -- discs dev [B][n_keep][3] or None (no discs) behind the
        field; the result carries keep_mult [B][n_keep][N], the discs' duals.  hard_moving: the moving discs are HARD (d2d_nlp_solve_keepout_moving,
        d2d_nlp_solve_groups_keepout): kwork follows mov_work, and the result carries keep_mult [B][n_mov][N].  fence: the entry is
        d2d_nlp_solve_fence -- edges dev [B][n_edge][4] or None (no edges) behind keep -- or, with n_ac, d2d_nlp_solve_groups_fence -- edges
        dev [R][n_edge][4], one polygon per scenario, behind the field; the result carries fence_mult [B][n_edge][N]."""
        torch = _torch()
        B, _, N = W.shape
        groups = n_ac is not None
        assert W.is_contiguous() and scen.shape[0] == B and (not groups or B % n_ac == 0)
        G = B // n_ac if groups else B
        ws = self.lib.d2d_nlp_workspace_doubles(N) if free_rows is None else self.lib.d2d_nlp_free_workspace_doubles(N)
        m = None if moving is _ABSENT else self._moving_c(*moving, G)
        v = None if via is _ABSENT else self._via_c(via, B)
        if field is not _ABSENT and not t_scalar:
            t_start = self._t_start_dev(t_start, G, W)
        work = self.empty((ws * n_ac + 2 * N) * G if groups else ws * B)
        cost, feas = self.empty(B), self.empty(B)
        iters = torch.empty(B, dtype=torch.int32, device=self.device); status = torch.empty(B, dtype=torch.int32, device=self.device)
        mult = self.zeros(B, 3, N) if want_mult else None
        assert bounds is None or (bounds.is_contiguous() and tuple(bounds.shape) == (B, 4) and bounds.dtype == torch.float64)
        assert order is None or (order.is_contiguous() and tuple(order.shape) == (B,) and order.dtype == torch.int32)
        o = NlpOpts(*opts, int(slots), None if bounds is None else bounds.data_ptr(), None if order is None else order.data_ptr())
        out = dict(cost=cost, feas=feas, iters=iters, status=status, work=work)
        args = [_ptr(work), _ptr(mult), _ptr(cost), _ptr(feas), _ptr(iters), _ptr(status)]
        if groups:
            out['sweeps'], out['moved'] = torch.empty(G, dtype=torch.int32, device=self.device), self.empty(G)
            args = [self.h, G, n_ac, N, float(h), _ptr(scen), C.byref(o), int(sweeps[0]), float(sweeps[1]), _ptr(W)] + args + [_ptr(out['sweeps']), _ptr(out['moved'])]
        elif free_rows is not None:
            assert free_rows.is_contiguous() and tuple(free_rows.shape) == (B, 4) and free_rows.dtype == torch.float64
            out['h'] = self.empty(B)
            args = [self.h, B, N, float(h), _ptr(scen), C.byref(o), _ptr(free_rows), _ptr(W)] + args + [_ptr(out['h'])]
        else:
            args = [self.h, B, N, float(h), _ptr(scen), C.byref(o), _ptr(W), *mid] + args
        if field is not _ABSENT:
            f = None if field is None else _wind_c(self, field)
            args += [None if f is None else C.byref(f), float(t_start) if t_scalar else _ptr(t_start)]
            if not t_scalar:
                out['t_start'] = t_start
            if groups:
                # prev [R][2][N]: the kernel's scratch behind the workspaces; it is left holding the x, y planes aircraft 1 had BEFORE its
                # last turn, i.e. the frozen partner that aircraft 0's last solve (and its reported cost) saw
                out['prev'] = work[ws * n_ac * G:].view(G, 2, N)
        if m is not None:
            out['mov_work'] = self.empty(G, m.n_mov, 2, N) if m.n_mov > 0 else None
            args += [C.byref(m), _ptr(out['mov_work'])]
            if hard_moving:
                out['keep_mult'] = self.zeros(B, m.n_mov, N) if m.n_mov > 0 else None
                args += [_ptr(out['keep_mult'])]
        if v is not None:
            out['via_work'] = torch.zeros(B, N, dtype=torch.int32, device=self.device) if v.n_via > 0 else None
            args += [C.byref(v), _ptr(out['via_work'])]
        if keep is not _ABSENT:
            assert keep is None or (keep.is_contiguous() and keep.dtype == torch.float64 and keep.dim() == 3 and keep.shape[0] == B and keep.shape[2] == 3)
            k = KeepOutC(0 if keep is None else int(keep.shape[1]), 0, None if keep is None else keep.data_ptr())
            out['keep_mult'] = self.zeros(B, k.n_keep, N) if k.n_keep > 0 else None
            args += [C.byref(k), _ptr(out['keep_mult'])]
        if fence is not _ABSENT:
            assert fence is None or (fence.is_contiguous() and fence.dtype == torch.float64 and fence.dim() == 3 and fence.shape[0] == G and fence.shape[2] == 4)
            fc = FenceC(0 if fence is None else int(fence.shape[1]), 0, None if fence is None else fence.data_ptr())
            out['fence_mult'] = self.zeros(B, fc.n_edge, N) if fc.n_edge > 0 else None
            args += [C.byref(fc), _ptr(out['fence_mult'])]
        _check(entry(*args))
        if want_mult:
            out['mult'] = mult
        return out

    def nlp_solve(self, scen, W, h, partner=None, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX,
                  outer_max=NLP_OUTER_MAX, want_mult=False, serial=0, bounds=None, slots=0, order=None):
        """Direct-collocation NLP in node variables (d2d_nlp_solve): scen dev [B][SCEN_STRIDE], W dev [B][5][N] in/out (initial
        guess -> solution), partner dev [B][2][N] or None, bounds dev [B][4] = (phi_lo, phi_hi, psi_lo, psi_hi) or None (d2d_nlp_opts.bounds),
        order dev int32 [B]: the hand-out order of the persistent launch (a permutation; d2d_nlp_opts.order) or None.
        Returns dict(cost, feas, iters, status[, mult [B][3][N]]) of device tensors."""
        B, _, N = W.shape
        assert partner is None or (partner.is_contiguous() and partner.shape == (B, 2, N))
        return self._nlp_core(self.lib.d2d_nlp_solve, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial), bounds,
                              want_mult=want_mult, slots=slots, order=order, mid=(_ptr(partner),))

    def nlp_guess_dubins(self, scen, N, h, bounds=None, v_pref=None, kappa=GUESS_KAPPA, W=None, outputs=None, waves=0):
        """The start of a collocation solve from a Dubins path (d2d_nlp_guess_dubins; tests/nlp_guess_ref.py is its CPU statement): scen
        dev [B][SCEN_STRIDE], N nodes of step h; bounds dev [B][4] as nlp_solve's or None; v_pref dev [B] or None (the rows' VSP / VREF);
        kappa: the fraction of the bank limit the arcs use.  W: dev [B][5][N] to fill (a refused row keeps its values) or None (zeros).
        Returns (W, dict of device tensors: status, word int32 [B] (GUESS_STATUS, GUESS_WORDS; word -1: none), v, rho, L, t_nat [B]).
        t_nat is a suggestion for nlp_solve_free's start step, t_nat / (N - 1), not a lower bound on the duration.  outputs: the names
        to compute (None: all six).  waves only schedules: the same bytes for every value."""
        torch = _torch()
        assert scen.dim() == 2 and scen.shape[1] == SCEN_STRIDE and scen.is_contiguous() and scen.dtype == torch.float64 and scen.device.type == 'cuda'
        B, N = scen.shape[0], int(N)
        assert bounds is None or (bounds.is_contiguous() and tuple(bounds.shape) == (B, 4) and bounds.dtype == torch.float64)
        assert v_pref is None or (v_pref.is_contiguous() and tuple(v_pref.shape) == (B,) and v_pref.dtype == torch.float64)
        if W is None:
            W = self.zeros(B, 5, max(N, 0))
        assert W.is_contiguous() and tuple(W.shape) == (B, 5, N) and W.dtype == torch.float64
        i32 = lambda: torch.empty(B, dtype=torch.int32, device=self.device)     # noqa: E731
        out = dict(status=i32(), word=i32(), v=self.empty(B), rho=self.empty(B), L=self.empty(B), t_nat=self.empty(B))
        if outputs is not None:
            unknown = set(outputs) - set(GUESS_OUT)
            if unknown:
                raise ValueError(f'outputs: unknown names {sorted(unknown)}')
            out = {k: v for k, v in out.items() if k in outputs}
        o = NlpGuessOut(**{k: v.data_ptr() for k, v in out.items()})
        opts = NlpGuessOpts(float(kappa), None if bounds is None else bounds.data_ptr(), None if v_pref is None else v_pref.data_ptr(), int(waves), 0)
        _check(self.lib.d2d_nlp_guess_dubins(self.h, B, N, float(h), _ptr(scen), C.byref(opts), _ptr(W), C.byref(o)))
        return W, out

    def nlp_solve_free(self, scen, W, h, free_rows, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX,
                       outer_max=NLP_OUTER_MAX, want_mult=False, bounds=None, slots=0, order=None):
        """nlp_solve with every problem's time step free (d2d_nlp_solve_free; opty's variable-duration Problem): free_rows dev [B][4] =
        (h_lo, h_hi, k_dur, h_start; 0 = h), the hard box of the step, the weight of the duration (N - 1) h in the objective and the
        start step.  No partner; the rows' constant wind.  Returns nlp_solve's dict plus h (device [B]: the solved steps; NaN for a
        refused problem); cost includes k_dur (N - 1) h."""
        return self._nlp_core(self.lib.d2d_nlp_solve_free, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, 0), bounds,
                              want_mult=want_mult, slots=slots, order=order, free_rows=free_rows)

    def nlp_solve_wind(self, scen, W, h, field, t_start=0.0, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7,
                       inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, want_mult=False, serial=0, bounds=None, slots=0, order=None):
        """nlp_solve with the wind of the equalities read from `field` (a d2d.wind.SplineWindField or a WindFieldC) at every node's own
        (t_start + i h, x_i, y_i) instead of the rows' constant (d2d_nlp_solve_wind; no partner).  The model ADDS the field to its
        residual: a plan for a plant that flies F is solved in -F.  Returns dict(cost, feas, iters, status[, mult]) of device tensors."""
        return self._nlp_core(self.lib.d2d_nlp_solve_wind, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial), bounds,
                              want_mult=want_mult, slots=slots, order=order, field=field, t_start=t_start, t_scalar=True)

    def nlp_solve_groups(self, scen, W, h, n_ac, max_sweeps=12, tol=1e-7, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7,
                         inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, serial=0, bounds=None):
        """The reference's multi-aircraft Problem for R scenarios in one launch (d2d_nlp_solve_groups): scen dev [R*n_ac][SCEN_STRIDE],
        W dev [R*n_ac][5][N] in/out, the aircraft of a scenario consecutive; CostCollision couples aircraft 0 and 1 (rows' KCOL > 0).
        Returns dict(cost, feas, iters, status per aircraft; sweeps, moved per scenario) of device tensors."""
        return self._nlp_core(self.lib.d2d_nlp_solve_groups, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial), bounds,
                              n_ac=n_ac, sweeps=(max_sweeps, tol))

    def nlp_solve_groups_wind(self, scen, W, h, n_ac, field, t_start, max_sweeps=12, tol=1e-7, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9,
                              opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, serial=0, bounds=None):
        """nlp_solve_groups with the wind of the equalities read from `field` (a d2d.wind.SplineWindField or a WindFieldC) at every
        node's own (t_start[r] + i h, x_i, y_i) instead of the rows' constant (d2d_nlp_solve_groups_wind).  t_start: device float64 [R],
        one start time per scenario (a float is spread over the scenarios).  The model ADDS the field to its residual: a plan for a
        plant that flies F is solved in -F.  Returns nlp_solve_groups's dict plus t_start and prev [R][2][N] (coupled scenarios: the
        positions of aircraft 1 before its last turn -- the partner the reported cost of aircraft 0 was evaluated against)."""
        return self._nlp_core(self.lib.d2d_nlp_solve_groups_wind, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial),
                              bounds, n_ac=n_ac, sweeps=(max_sweeps, tol), field=field, t_start=t_start)

    def nlp_solve_groups_pairs(self, scen, W, h, n_ac, field=None, t_start=None, max_sweeps=12, tol=1e-7, rho0=10.0, mub0=0.1, mub_min=1e-9,
                               feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, serial=0, bounds=None):
        """nlp_solve_groups / nlp_solve_groups_wind with CostCollision on any set of pairs (d2d_nlp_solve_groups_pairs): SC_PMASK of
        aircraft a's row is its partner set (bit j: aircraft j of the scenario), and every aircraft with a partner takes turns against
        the frozen positions of all of them.  field None: the rows' constant wind (t_start is not read); else as nlp_solve_groups_wind.
        A scenario with a malformed mask (no integer in [0, 2^n_ac), a self bit, a bit its partner does not return) is refused on the
        device: status ST_NONFINITE, cost = feas = NaN, sweeps 0, its W untouched.  Returns nlp_solve_groups_wind's dict."""
        if field is None:
            t_start = None
        elif t_start is None:
            t_start = 0.0
        return self._nlp_core(self.lib.d2d_nlp_solve_groups_pairs, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial),
                              bounds, n_ac=n_ac, sweeps=(max_sweeps, tol), field=field, t_start=t_start)

    def _moving_c(self, knots, disc, G):
        """d2d_moving_obstacles over device tables: knots [G][n_mov][n_knot][3] and disc [G][n_mov][2], or (None, None): nothing moves.
        Shapes only -- the ranges are the library's to check (D2D_EINVAL) and the tracks' contents the kernels'."""
        torch = _torch()
        if knots is None and disc is None:
            return MovingObstaclesC(0, 0, None, None)
        for t in (knots, disc):
            assert t.is_contiguous() and t.dtype == torch.float64 and t.device.type == 'cuda'
        assert knots.dim() == 4 and knots.shape[0] == G and knots.shape[3] == 3 and tuple(disc.shape) == (G, knots.shape[1], 2)
        return MovingObstaclesC(int(knots.shape[1]), int(knots.shape[2]), knots.data_ptr(), disc.data_ptr())

    def _t_start_dev(self, t_start, G, ref):
        torch = _torch()
        if t_start is not None and not torch.is_tensor(t_start):
            t_start = torch.full((G,), float(t_start), dtype=torch.float64, device=self.device)
        assert t_start is None or (t_start.is_contiguous() and tuple(t_start.shape) == (G,) and t_start.dtype == torch.float64 and t_start.device == ref.device)
        return t_start

    def mov_sample(self, knots, disc, t_start, N, h):
        """The centres of moving discs at the node times (d2d_mov_sample): knots dev [G][n_mov][n_knot][3], disc dev [G][n_mov][2],
        t_start dev [G] (or a float) -> ctr dev [G][n_mov][2][N], disc m of problem g at t_start[g] + i h."""
        G = knots.shape[0]
        m = self._moving_c(knots, disc, G)
        t_start = self._t_start_dev(t_start, G, knots)
        ctr = self.empty(G, m.n_mov, 2, int(N))
        _check(self.lib.d2d_mov_sample(self.h, G, int(N), float(h), _ptr(t_start), C.byref(m), _ptr(ctr)))
        return ctr

    def nlp_solve_moving(self, scen, W, h, knots=None, disc=None, field=None, t_start=None, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9,
                         opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, want_mult=False, serial=0, bounds=None, slots=0,
                         order=None):
        """nlp_solve / nlp_solve_wind around moving discs (d2d_nlp_solve_moving): knots dev [B][n_mov][n_knot][3] = (t, x, y) and disc
        dev [B][n_mov][2] = (r, kind) per problem (both None: nothing moves), field None: the rows' constant wind, t_start dev [B] or a
        float: the problems' start times (required when discs move or with a field).  A problem with an unusable track or start time is
        refused on the device: status ST_NONFINITE, cost = feas = NaN, its W untouched.  Returns nlp_solve's dict plus mov_work
        [B][n_mov][2][N]: the discs' centres at the node times."""
        return self._nlp_core(self.lib.d2d_nlp_solve_moving, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial), bounds,
                              want_mult=want_mult, slots=slots, order=order, field=field, t_start=t_start, moving=(knots, disc))

    def nlp_solve_groups_moving(self, scen, W, h, n_ac, knots=None, disc=None, field=None, t_start=None, max_sweeps=12, tol=1e-7, rho0=10.0,
                                mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, serial=0,
                                bounds=None):
        """nlp_solve_groups_pairs around moving discs (d2d_nlp_solve_groups_moving): knots dev [R][n_mov][n_knot][3] and disc dev
        [R][n_mov][2] per SCENARIO -- all its aircraft see the same tracks -- and t_start dev [R] or a float (required when discs move
        or with a field).  A scenario with an unusable track is refused like one with a malformed mask.  Returns
        nlp_solve_groups_pairs's dict plus mov_work [R][n_mov][2][N]."""
        return self._nlp_core(self.lib.d2d_nlp_solve_groups_moving, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial),
                              bounds, n_ac=n_ac, sweeps=(max_sweeps, tol), field=field, t_start=t_start, moving=(knots, disc))

    def nlp_solve_keepout(self, scen, W, h, discs, field=None, t_start=None, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7,
                          inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, want_mult=False, serial=0, bounds=None, slots=0, order=None):
        """nlp_solve / nlp_solve_wind outside HARD keep-out discs (d2d_nlp_solve_keepout): discs dev [B][n_keep][3] = (cx, cy, R) per
        problem (R <= 0: absent; None: no discs), every interior node held at |p - c|^2 - R^2 > 0 by the solver's barrier.  field None: the
        rows' constant wind (t_start is not read); else t_start dev [B] or a float.  A problem with a non-finite disc, an end pose on or
        inside a disc, or no start outside its discs is refused on the device: status ST_NONFINITE, cost = feas = NaN, its W untouched.
        Returns nlp_solve's dict plus keep_mult [B][n_keep][N]: the multipliers of the disc constraints."""
        if field is None:
            t_start = None
        elif t_start is None:
            t_start = 0.0
        return self._nlp_core(self.lib.d2d_nlp_solve_keepout, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial), bounds,
                              want_mult=want_mult, slots=slots, order=order, field=field, t_start=t_start, keep=discs)

    def nlp_solve_fence(self, scen, W, h, edges, discs=None, field=None, t_start=None, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9,
                        opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, want_mult=False, serial=0, bounds=None, slots=0,
                        order=None):
        """nlp_solve_keepout INSIDE a convex polygon (d2d_nlp_solve_fence): edges dev [B][n_edge][4] = (ax, ay, b, kap) per problem, a the
        outward unit normal (ax = ay = 0: absent; None: no edges; d2d.opty_utils.GeoFence.lowered() gives the rows), every interior node
        held at b - a . p > 0 by the solver's barrier; discs as nlp_solve_keepout's (None: none), held in the same solve.  Refused on the
        device (status ST_NONFINITE, cost = feas = NaN, W untouched): a non-finite edge, a normal off unit length, kap <= 0, an end pose
        on or outside an edge, no start inside the edges and outside the discs -- and nlp_solve_keepout's causes.  The feasible set is
        convex: the polyline between the returned nodes stays inside.  Returns nlp_solve_keepout's dict plus fence_mult [B][n_edge][N]:
        the multipliers of the edge constraints."""
        if field is None:
            t_start = None
        elif t_start is None:
            t_start = 0.0
        return self._nlp_core(self.lib.d2d_nlp_solve_fence, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial), bounds,
                              want_mult=want_mult, slots=slots, order=order, field=field, t_start=t_start, keep=discs, fence=edges)

    def nlp_solve_free_fence(self, scen, W, h, free_rows, discs=None, edges=None, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7,
                             inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, want_mult=False, bounds=None, slots=0, order=None):
        """nlp_solve_free outside static HARD discs and inside a convex polygon (d2d_nlp_solve_free_fence): the leg's duration is free
        while both families are held.  free_rows as nlp_solve_free's; discs dev [B][n_keep][3] as nlp_solve_keepout's and edges dev
        [B][n_edge][4] as nlp_solve_fence's (None: none; both None: nlp_solve_free's kernel and bytes).  The rows' constant wind; no
        field, nothing moves, no pins.  Refused on the device (ST_NONFINITE, cost = feas = h = NaN, W untouched): nlp_solve_free's
        causes and nlp_solve_fence's.  The discs are held at the nodes: inflate R for the chord with the LARGEST step of the box.
        Returns nlp_solve_free's dict plus keep_mult [B][n_keep][N] and fence_mult [B][n_edge][N], as nlp_solve_fence."""
        return self._nlp_core(self.lib.d2d_nlp_solve_free_fence, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, 0), bounds,
                              want_mult=want_mult, slots=slots, order=order, free_rows=free_rows, keep=discs, fence=edges)

    def nlp_solve_groups_fence(self, scen, W, h, n_ac, edges, field=None, t_start=None, max_sweeps=12, tol=1e-7, rho0=10.0, mub0=0.1, mub_min=1e-9,
                               feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, serial=0, bounds=None, want_mult=False):
        """nlp_solve_groups_pairs with every aircraft inside its scenario's convex polygon (d2d_nlp_solve_groups_fence): edges dev
        [R][n_edge][4] per SCENARIO, read as nlp_solve_fence reads them (None: no edges, nlp_solve_groups_pairs).  No hard discs.  A
        scenario with an unusable edge, or with an aircraft whose end pose lies on or outside an edge or that cannot be started inside,
        is refused like one with a malformed mask.  Returns nlp_solve_groups_pairs's dict plus fence_mult [R*n_ac][n_edge][N]: every
        aircraft's multipliers."""
        if field is None:
            t_start = None
        elif t_start is None:
            t_start = 0.0
        return self._nlp_core(self.lib.d2d_nlp_solve_groups_fence, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial),
                              bounds, n_ac=n_ac, sweeps=(max_sweeps, tol), want_mult=want_mult, field=field, t_start=t_start, fence=edges)

    def nlp_solve_keepout_moving(self, scen, W, h, knots=None, disc=None, field=None, t_start=None, rho0=10.0, mub0=0.1, mub_min=1e-9,
                                 feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, want_mult=False, serial=0,
                                 bounds=None, slots=0, order=None):
        """nlp_solve_keepout outside hard discs that MOVE (d2d_nlp_solve_keepout_moving): the tables of nlp_solve_moving, knots dev
        [B][n_mov][n_knot][3] = (t, x, y) and disc dev [B][n_mov][2] = (R, kind) with R the NODE RADIUS of the hard constraint (R <= 0:
        absent; the kind is validated and not read).  Every interior node i is held at |p_i - c(t_start + i h)|^2 - R^2 > 0.  t_start dev
        [B] or a float is required when discs are given.  Refused on the device (status ST_NONFINITE, cost = feas = NaN, W untouched): an
        unusable track or start time, a non-finite R, an end pose on or inside a disc at its own node's time, no start outside the discs.
        Returns nlp_solve_moving's dict plus keep_mult [B][n_mov][N]: the multipliers of the disc constraints."""
        return self._nlp_core(self.lib.d2d_nlp_solve_keepout_moving, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial),
                              bounds, want_mult=want_mult, slots=slots, order=order, field=field, t_start=t_start, moving=(knots, disc),
                              hard_moving=True)

    def nlp_solve_groups_keepout(self, scen, W, h, n_ac, knots=None, disc=None, field=None, t_start=None, max_sweeps=12, tol=1e-7, rho0=10.0,
                                 mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, serial=0,
                                 bounds=None):
        """nlp_solve_groups_pairs with every aircraft outside its scenario's hard moving discs (d2d_nlp_solve_groups_keepout): knots dev
        [R][n_mov][n_knot][3] and disc dev [R][n_mov][2] = (R, kind) per SCENARIO, read as nlp_solve_keepout_moving reads them.  A
        scenario with an unusable track, radius or start time, or with an aircraft whose end pose lies inside a disc or that cannot be
        started outside the discs, is refused like one with a malformed mask.  Returns nlp_solve_groups_moving's dict plus keep_mult
        [R*n_ac][n_mov][N]: every aircraft's multipliers."""
        return self._nlp_core(self.lib.d2d_nlp_solve_groups_keepout, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial),
                              bounds, n_ac=n_ac, sweeps=(max_sweeps, tol), field=field, t_start=t_start, moving=(knots, disc), hard_moving=True)

    def _via_c(self, via, G):
        """d2d_via_points over a device table [G][n_via][5] = (node, mask, x, y, psi), or None: no pins.  Shapes only -- the range of
        n_via is the library's to check (D2D_EINVAL) and the rows' contents the kernels'."""
        torch = _torch()
        if via is None:
            return ViaPointsC(0, None)
        assert via.is_contiguous() and via.dtype == torch.float64 and via.device.type == 'cuda'
        assert via.dim() == 3 and via.shape[0] == G and via.shape[2] == 5
        return ViaPointsC(int(via.shape[1]), via.data_ptr())

    def nlp_solve_via(self, scen, W, h, via, knots=None, disc=None, field=None, t_start=None, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9,
                      opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, want_mult=False, serial=0, bounds=None, slots=0,
                      order=None):
        """nlp_solve_moving through timed waypoints (d2d_nlp_solve_via): via dev [B][n_via][5] = (node, mask, x, y, psi) per problem,
        mask bits 0..2 = x, y, psi of that node pinned, a row of mask 0 absent (None: no pins); the other arguments as nlp_solve_moving.
        A problem with an unusable row (node outside 1 .. N-2, mask outside 0 .. 7, a non-finite or out-of-box value, a component pinned
        twice) is refused on the device: status ST_NONFINITE, cost = feas = NaN, its W untouched.  The pinned components of the returned
        W hold their values exactly.  Returns nlp_solve_moving's dict plus via_work int32 [B][N]: the fixed set of every node."""
        return self._nlp_core(self.lib.d2d_nlp_solve_via, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial), bounds,
                              want_mult=want_mult, slots=slots, order=order, field=field, t_start=t_start, moving=(knots, disc), via=via)

    def nlp_solve_groups_via(self, scen, W, h, n_ac, via, knots=None, disc=None, field=None, t_start=None, max_sweeps=12, tol=1e-7, rho0=10.0,
                             mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX, outer_max=NLP_OUTER_MAX, serial=0,
                             bounds=None, want_mult=False):
        """nlp_solve_groups_moving through timed waypoints (d2d_nlp_solve_groups_via): via dev [R*n_ac][n_via][5], every AIRCRAFT its own
        rows (None: no pins); knots / disc per scenario as before.  An unusable row of any aircraft refuses its whole scenario, like a
        malformed mask.  Returns nlp_solve_groups_moving's dict plus via_work int32 [R*n_ac][N] and, with want_mult, mult [R*n_ac][3][N]:
        the scaled multiplier estimates of every aircraft's last solve."""
        return self._nlp_core(self.lib.d2d_nlp_solve_groups_via, scen, W, h, (rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial),
                              bounds, n_ac=n_ac, sweeps=(max_sweeps, tol), want_mult=want_mult, field=field, t_start=t_start, moving=(knots, disc),
                              via=via)

    def nlp_solve_model(self, scen, W, h, g, H, Wc, rho0=10.0, mub0=0.1, mub_min=1e-9, feas_tol=1e-9, opt_tol=1e-7, inner_max=NLP_INNER_MAX,
                        outer_max=NLP_OUTER_MAX, want_mult=False, serial=0, bounds=None):
        """The collocation NLP under a quadratic objective model (d2d_nlp_solve_model): minimise sum_i g_i.d_i + 1/2 d_i^T H_i d_i,
        d_i = W_i - Wc_i, over the feasible set of scen's rows (their cost weights are the caller's business: the host-objective path
        zeroes them).  g, Wc dev [B][5][N], H dev [B][15][N] (upper triangle of each node's 5x5 block, row by row), W dev [B][5][N]
        in/out, bounds as nlp_solve.  Returns dict(cost (the model's value at the solution), feas, iters, status[, mult]) of device tensors."""
        torch = _torch()
        B, _, N = W.shape
        assert W.is_contiguous() and scen.shape[0] == B
        for t, k in ((g, 5), (H, 15), (Wc, 5)):
            assert t.is_contiguous() and tuple(t.shape) == (B, k, N) and t.dtype == torch.float64 and t.device == W.device
        work = self.empty(self.lib.d2d_nlp_workspace_doubles(N) * B)
        cost, feas = self.empty(B), self.empty(B)
        iters = torch.empty(B, dtype=torch.int32, device=self.device); status = torch.empty(B, dtype=torch.int32, device=self.device)
        mult = self.zeros(B, 3, N) if want_mult else None
        assert bounds is None or (bounds.is_contiguous() and tuple(bounds.shape) == (B, 4) and bounds.dtype == torch.float64)
        o = NlpOpts(rho0, mub0, mub_min, feas_tol, opt_tol, inner_max, outer_max, serial, 0, None if bounds is None else bounds.data_ptr(), None)
        m = NlpModel(g.data_ptr(), H.data_ptr(), Wc.data_ptr())
        _check(self.lib.d2d_nlp_solve_model(self.h, B, N, float(h), _ptr(scen), C.byref(o), C.byref(m), _ptr(W), _ptr(work), _ptr(mult),
                                            _ptr(cost), _ptr(feas), _ptr(iters), _ptr(status)))
        out = dict(cost=cost, feas=feas, iters=iters, status=status, work=work)
        if want_mult:
            out['mult'] = mult
        return out

    def flight_audit(self, X_hist, n_ac, dt_row, rows=None, t_start=None, x_ref=None, y_ref=None, static=None, knots=None, disc=None,
                     d_safe=0.0, err_tol=float('inf'), rows_per_block=0, layout='hist', outputs=None):
        """Audit a state history that is on the device (d2d_flight_audit): X_hist dev [n_rows][5][N], N = n_form * n_ac, row i of
        formation f at t_start[f] + i dt_row (t_start dev [n_form], a float or None: 0).  layout='plan': X_hist is a collocation plan
        W [N][5][K], transposed here to [K][5][N].  rows dev int32 [n_form]: the valid rows (None: all).  x_ref, y_ref dev [n_rows][N]:
        the tracked reference (both or neither).  static dev [n_form][n_stat][3] = (x, y, r): static discs; knots, disc: the tables of
        Context.mov_sample with G = n_form (t_start is then required).  Returns a dict of device tensors, per drone [N]: sep_dist,
        sep_partner, sep_time, sep_count (rows closer than d_safe); stat_* / mov_* [n_disc][N]: clear, time, count; err_max, err_time,
        err_count (rows above err_tol); phi_max, v_min, v_max; status int32 [n_form] (0, or the AUDIT_* bits of a refused formation:
        its floating outputs are NaN, its counts -1); mov_work [n_form][n_mov][2][n_rows]: the moving centres at the rows.  The result
        does not depend on rows_per_block (0: the library's choice), bit for bit.  outputs: the groups to compute, of 'sep', 'env'
        (phi_max, v_min, v_max), 'err', 'stat', 'mov' (None: every group the inputs allow); only the planes they need are read."""
        torch = _torch()
        if layout == 'plan':
            X_hist = X_hist.permute(2, 1, 0).contiguous()
        elif layout != 'hist':
            raise ValueError(f"layout={layout!r}: 'hist' ([n_rows][5][N]) or 'plan' ([N][5][K])")
        assert X_hist.dim() == 3 and X_hist.shape[1] == 5 and X_hist.is_contiguous() and X_hist.dtype == torch.float64 and X_hist.device.type == 'cuda'
        n_rows, _, N = X_hist.shape
        n_ac = int(n_ac)
        n_form = N // n_ac if n_ac >= 1 else 0
        assert n_ac < 1 or N == n_form * n_ac
        for t in (x_ref, y_ref):
            assert t is None or (t.is_contiguous() and tuple(t.shape) == (n_rows, N) and t.dtype == torch.float64 and t.device == X_hist.device)
        assert rows is None or (rows.is_contiguous() and tuple(rows.shape) == (n_form,) and rows.dtype == torch.int32 and rows.device == X_hist.device)
        assert static is None or (static.is_contiguous() and static.dim() == 3 and static.shape[0] == n_form and static.shape[2] == 3
                                  and static.dtype == torch.float64 and static.device == X_hist.device)
        n_stat = 0 if static is None else int(static.shape[1])
        m = self._moving_c(knots, disc, n_form)
        t_start = self._t_start_dev(t_start, n_form, X_hist)
        p = AuditParams(n_form, n_ac, n_rows, int(rows_per_block), n_stat, 0, float(dt_row), float(d_safe), float(err_tol))
        nbytes = self.lib.d2d_flight_audit_workspace(C.byref(p), m.n_mov)
        if nbytes < 0:
            _check(int(nbytes))
        work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        mov_work = self.empty(n_form, m.n_mov, 2, n_rows) if m.n_mov > 0 else None
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=self.device)     # noqa: E731
        out = dict(sep_dist=self.empty(N), sep_partner=i32(N), sep_time=self.empty(N), sep_count=i32(N), phi_max=self.empty(N),
                   v_min=self.empty(N), v_max=self.empty(N), status=i32(n_form))
        if n_stat > 0:
            out.update(stat_clear=self.empty(n_stat, N), stat_time=self.empty(n_stat, N), stat_count=i32(n_stat, N))
        if m.n_mov > 0:
            out.update(mov_clear=self.empty(m.n_mov, N), mov_time=self.empty(m.n_mov, N), mov_count=i32(m.n_mov, N))
        if x_ref is not None and y_ref is not None:
            out.update(err_max=self.empty(N), err_time=self.empty(N), err_count=i32(N))
        if outputs is not None:
            keep = {'sep': 'sep_', 'env': ('phi_', 'v_'), 'err': 'err_', 'stat': 'stat_', 'mov': 'mov_'}
            pre = tuple(x for g in outputs for x in np.atleast_1d(keep[g]))
            out = {k: v for k, v in out.items() if k == 'status' or k.startswith(pre)}
        o = AuditOut(**{k: v.data_ptr() for k, v in out.items()})
        _check(self.lib.d2d_flight_audit(self.h, C.byref(p), _ptr(X_hist), _ptr(rows), _ptr(t_start), _ptr(x_ref), _ptr(y_ref), _ptr(static),
                                         C.byref(m), _ptr(mov_work), _ptr(work), C.byref(o)))
        out['mov_work'] = mov_work                    # (work is released here: the context's stream is torch's, whose allocator orders its reuse)
        return out

    def fleet_audit(self, X_hist, n_ac, dt_row, d_look, step_max, rows=None, row0=None, world=None, d_safe=0.0, g_rows=None, tile_rows=0,
                    slots=0, layout='hist', outputs=None):
        """Audit the separation between aircraft of DIFFERENT formations (d2d_fleet_audit): X_hist dev [n_rows][5][N], N = n_form * n_ac
        (layout='plan': a collocation plan [N][5][K], transposed here).  rows dev int32 [n_form]: the valid rows (None: all); row0 dev
        int32 [n_form]: the global row of each formation's row 0 (None: 0); world dev int32 [n_form]: only formations of one world are
        compared (None: one world).  d_look (m): nothing farther is reported; step_max (m): the largest step of any aircraft between
        two rows, checked; d_safe (m, <= d_look): rows closer than it are counted.  g_rows: the global rows swept (None: n_rows
        without row0, else max(row0 + rows), read from the device).  Returns a dict of device tensors: near_dist, near_time (at
        (g + s) dt_row), near_partner (a global drone index), near_count [N]; status int32 [n_form] (0, or the FLEET_* bits of a
        refused formation: its floating outputs are NaN, its counts and partners -1, and no other formation sees it).  Nothing within
        d_look: +inf, -1, NaN, 0.  tile_rows and slots only schedule (0: the library's choice): the result is the same bits for
        every value.  outputs: the names to compute (None: all five)."""
        torch = _torch()
        if layout == 'plan':
            X_hist = X_hist.permute(2, 1, 0).contiguous()
        elif layout != 'hist':
            raise ValueError(f"layout={layout!r}: 'hist' ([n_rows][5][N]) or 'plan' ([N][5][K])")
        assert X_hist.dim() == 3 and X_hist.shape[1] == 5 and X_hist.is_contiguous() and X_hist.dtype == torch.float64 and X_hist.device.type == 'cuda'
        n_rows, _, N = X_hist.shape
        n_ac = int(n_ac)
        n_form = N // n_ac if n_ac >= 1 else 0
        assert n_ac < 1 or N == n_form * n_ac
        for t in (rows, row0, world):
            assert t is None or (t.is_contiguous() and tuple(t.shape) == (n_form,) and t.dtype == torch.int32 and t.device == X_hist.device)
        if g_rows is None:
            if row0 is None:
                g_rows = n_rows
            else:
                r = torch.full_like(row0, n_rows) if rows is None else torch.clamp(rows, 0, n_rows)
                g_rows = max(int((row0.to(torch.int64) + r).max().item()), 1)
        p = FleetParams(n_form, n_ac, n_rows, int(g_rows), int(tile_rows), int(slots), float(dt_row), float(d_look), float(step_max), float(d_safe))
        nbytes = self.lib.d2d_fleet_audit_workspace(C.byref(p))
        if nbytes < 0:
            _check(int(nbytes))
        work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=self.device)     # noqa: E731
        out = dict(near_dist=self.empty(N), near_partner=i32(N), near_time=self.empty(N), near_count=i32(N), status=i32(n_form))
        if outputs is not None:
            unknown = set(outputs) - set(FLEET_OUT)
            if unknown:
                raise ValueError(f'outputs: unknown names {sorted(unknown)}')
            out = {k: v for k, v in out.items() if k in outputs}
        o = FleetOut(**{k: v.data_ptr() for k, v in out.items()})
        _check(self.lib.d2d_fleet_audit(self.h, C.byref(p), _ptr(X_hist), _ptr(rows), _ptr(row0), _ptr(world), _ptr(work), C.byref(o)))
        return out                                    # (work is released here: the context's stream is torch's, whose allocator orders its reuse)

    def fleet_tracks(self, X_hist, n_ac, dt_row, d_look, step_max, r_disc, rows=None, row0=None, world=None, prio=None, n_mov=MAX_MOV, n_knot=MOV_MAX_KNOT,
                     kind=1, t0=0.0, g_rows=None, tile_rows=0, slots=0, layout='hist', outputs=None):
        """The aircraft every formation must give way to, as moving-obstacle tables (d2d_fleet_tracks).  The history arguments are those
        of fleet_audit (X_hist dev [n_rows][5][N], layout='plan': a collocation plan [N][5][K]; rows, row0, world dev int32 [n_form];
        d_look, step_max; g_rows).  prio dev int32 [n_form]: the formation with the smaller (prio, index) keeps its plan (None: the
        index).  Per formation the n_mov nearest aircraft of formations that outrank it, by the audit's candidates below d_look, are
        written as tracks of n_knot knots across the formation's own window, global row g at t0 + g dt_row, with discs (r_disc, kind).
        Returns a dict of device tensors: knots [n_form][n_mov][n_knot][3] and disc [n_form][n_mov][2] (the tables of
        nlp_solve_groups_moving with R = n_form; an absent slot has r = 0 and a valid dummy track), partner int32, part_dist, part_time,
        chord_err [n_form][n_mov] (partner -1: absent; chord_err: what the decimation to n_knot knots gives away, to be added to the
        radius), n_conf int32 [n_form] (the partners found, n_mov + 1: more than slots; -1: a formation with a status), status int32
        [n_form] (the FLEET_* bits and TRACKS_SHORT).  tile_rows and slots only schedule: the same bits for every value.  outputs: the
        names to compute (None: all)."""
        torch = _torch()
        if layout == 'plan':
            X_hist = X_hist.permute(2, 1, 0).contiguous()
        elif layout != 'hist':
            raise ValueError(f"layout={layout!r}: 'hist' ([n_rows][5][N]) or 'plan' ([N][5][K])")
        assert X_hist.dim() == 3 and X_hist.shape[1] == 5 and X_hist.is_contiguous() and X_hist.dtype == torch.float64 and X_hist.device.type == 'cuda'
        n_rows, _, N = X_hist.shape
        n_ac = int(n_ac)
        n_form = N // n_ac if n_ac >= 1 else 0
        assert n_ac < 1 or N == n_form * n_ac
        for t in (rows, row0, world, prio):
            assert t is None or (t.is_contiguous() and tuple(t.shape) == (n_form,) and t.dtype == torch.int32 and t.device == X_hist.device)
        if g_rows is None:
            if row0 is None:
                g_rows = n_rows
            else:
                r = torch.full_like(row0, n_rows) if rows is None else torch.clamp(rows, 0, n_rows)
                g_rows = max(int((row0.to(torch.int64) + r).max().item()), 1)
        n_mov, n_knot = int(n_mov), int(n_knot)
        p = FleetParams(n_form, n_ac, n_rows, int(g_rows), int(tile_rows), int(slots), float(dt_row), float(d_look), float(step_max), 0.0)
        nbytes = self.lib.d2d_fleet_tracks_workspace(C.byref(p), n_mov)
        if nbytes < 0:
            _check(int(nbytes))
        work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=self.device)     # noqa: E731
        kn = max(n_knot, 0)                           # (a bad n_knot is the library's to refuse)
        out = dict(knots=self.empty(n_form, n_mov, kn, 3), disc=self.empty(n_form, n_mov, 2), partner=i32(n_form, n_mov),
                   part_dist=self.empty(n_form, n_mov), part_time=self.empty(n_form, n_mov), chord_err=self.empty(n_form, n_mov),
                   n_conf=i32(n_form), status=i32(n_form))
        if outputs is not None:
            unknown = set(outputs) - set(TRACKS_OUT)
            if unknown:
                raise ValueError(f'outputs: unknown names {sorted(unknown)}')
            out = {k: v for k, v in out.items() if k in outputs}
        o = TracksOut(**{k: v.data_ptr() for k, v in out.items()})
        _check(self.lib.d2d_fleet_tracks(self.h, C.byref(p), _ptr(X_hist), _ptr(rows), _ptr(row0), _ptr(world), _ptr(prio), n_mov, n_knot,
                                         float(r_disc), int(kind), float(t0), _ptr(work), C.byref(o)))
        return out                                    # (work is released here: the context's stream is torch's, whose allocator orders its reuse)

    def wind_fit(self, X_hist, n_ac, dt_row, grid, rows=None, t_start=None, prior=None, w_max=50.0, lam=(1e-2, 1e-2, 1e-2), mu=1e-6,
                 cg_tol=1e-10, cg_max=2000, outputs=None, waves=0):
        """Fit a wind field to a state history that is on the device (d2d_wind_fit): X_hist dev [n_rows][5][N], N = n_form * n_ac, row i
        of formation f at t_start[f] + i dt_row (t_start dev [n_form], a float or None: 0); rows dev int32 [n_form]: the valid rows
        (None: all).  grid: a WindFieldC or an object with device_field(ctx) whose geometry (nt, ny, nx, knots) the estimate takes;
        its control points are not read.  prior: dev [nt][2][ny][nx] the estimate is pulled towards with weight mu (None: 0).  lam =
        (lam_x, lam_y, lam_t) or one number: the weights of the second differences.  outputs: of 'support', 'stats', 'H', 'b' (None:
        support and stats).  waves: wavefronts of the accumulation launch (0: the library's choice; the bits do not depend on it).
        Returns dict(cp dev [nt][2][ny][nx], field: a WindFieldC on cp, support dev [nt ny nx], stats dev [8] (WINDFIT_STATS),
        H dev [nt ny nx][49 or 343], b dev [2][nt ny nx])."""
        torch = _torch()
        assert X_hist.dim() == 3 and X_hist.shape[1] == 5 and X_hist.is_contiguous() and X_hist.dtype == torch.float64 and X_hist.device.type == 'cuda'
        n_rows, _, N = X_hist.shape
        n_ac = int(n_ac)
        n_form = N // n_ac if n_ac >= 1 else 0
        assert n_ac < 1 or N == n_form * n_ac
        assert rows is None or (rows.is_contiguous() and tuple(rows.shape) == (n_form,) and rows.dtype == torch.int32 and rows.device == X_hist.device)
        t_start = self._t_start_dev(t_start, n_form, X_hist)
        g0 = _wind_c(self, grid)
        nt, ny, nx = int(g0.nt), int(g0.ny), int(g0.nx)
        shape = (max(nt, 0), 2, max(ny, 0), max(nx, 0))
        assert prior is None or (prior.is_contiguous() and tuple(prior.shape) == shape and prior.dtype == torch.float64 and prior.device == X_hist.device)
        g = WindFieldC(nt, ny, nx, 0, g0.t0, g0.ht, g0.x0, g0.hx, g0.y0, g0.hy, None if prior is None else prior.data_ptr())
        lam = (float(lam),) * 3 if np.ndim(lam) == 0 else tuple(float(v) for v in lam)
        p = WindFitParams(n_form, n_ac, n_rows, int(cg_max), int(waves), 0, float(dt_row), float(w_max), lam[0], lam[1], lam[2], float(mu),
                          float(cg_tol))
        nbytes = self.lib.d2d_wind_fit_workspace(C.byref(p), C.byref(g))
        if nbytes < 0:
            _check(int(nbytes))
        ncp = nt * ny * nx
        work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        cp = self.empty(*shape)
        want = ('support', 'stats') if outputs is None else tuple(outputs)
        unknown = set(want) - {'support', 'stats', 'H', 'b'}
        if unknown:
            raise ValueError(f'outputs: unknown names {sorted(unknown)}')
        out = dict(support=self.empty(ncp) if 'support' in want else None, stats=self.zeros(8) if 'stats' in want else None,
                   H=self.empty(ncp, 49 if nt == 1 else 343) if 'H' in want else None, b=self.empty(2, ncp) if 'b' in want else None)
        o = WindFitOut(_ptr(out['support']), _ptr(out['stats']), _ptr(out['H']), _ptr(out['b']))
        _check(self.lib.d2d_wind_fit(self.h, C.byref(p), _ptr(X_hist), _ptr(rows), _ptr(t_start), C.byref(g), _ptr(cp), _ptr(work), C.byref(o)))
        out = {k: v for k, v in out.items() if v is not None}
        out['cp'] = cp
        out['field'] = WindFieldC(nt, ny, nx, 0, g0.t0, g0.ht, g0.x0, g0.hx, g0.y0, g0.hy, cp.data_ptr())
        return out                                    # (work is released here: the context's stream is torch's, whose allocator orders its reuse)

    def track_run(self, x_ref, y_ref, X0, dt, record=('X', 'U', 'Xr', 'dX', 'Yd', 'Ydd'), out=None, wind=None, t_start=0.0, gust=None,
                  gust_state=None, gust_phase=0, gust_n_ac=1, gust_stream_base=0, **kw):
        """x_ref, y_ref dev [T][n]; X0 dev [5][n] -> dict of device histories (out: reuse the buffers of an earlier
        call with the same shapes and `record`).  wind: a field the plant flies (d2d_sim_track_run_wind; the controller keeps the
        constant w of kw; row i at t_start + i dt); out['iter_max']: the largest fixed-point sweep count.  t_start: a float, or a
        device float64 tensor [n] with every drone's own start time (d2d_sim_track_run_wind_at).  gust: a d2d.wind.GustModel the plant
        flies on top of w or the field (d2d_sim_track_run_gust; gust_state dev [4][n] or None, gust_phase, gust_stream_base as in gvf_run;
        gust_n_ac: consecutive drones that share the formation part); out['gust_state'] dev [4][n] and, with 'g' in record, out['g']
        dev [T][2][n].  gust None: nothing new is launched."""
        T, n = x_ref.shape
        p = self.track_params(n, T, dt, **kw)
        if out is None:
            out = {k: (self.zeros(T, c, n) if k in record else None)
                   for k, c in (('X', 5), ('U', 2), ('Xr', 5), ('dX', 5), ('Yd', 2), ('Ydd', 2))}
            out['X_final'] = self.empty(5, n)
        else:
            assert out['X_final'].shape == (5, n) and all(out[k] is None or out[k].shape[0] == T for k in ('X', 'U', 'Xr', 'dX', 'Yd', 'Ydd'))
        args = (self.h, C.byref(p), _ptr(x_ref), _ptr(y_ref), _ptr(X0), _ptr(out['X']), _ptr(out['U']), _ptr(out['Xr']), _ptr(out['dX']),
                _ptr(out['Yd']), _ptr(out['Ydd']), _ptr(out['X_final']))
        f, t_at, g = self._plant_extras(out, n, T, record, wind, gust, (dt, gust_n_ac, gust_phase, gust_state, gust_stream_base), t_start)
        if g is not None:
            if f is not None and t_at is None and float(t_start) != 0.0:     # (the entry point takes the start times per drone, or none: all 0)
                t_at = _torch().full((n,), float(t_start), dtype=_torch().float64, device=self.device)
            _check(self.lib.d2d_sim_track_run_gust(*args, None if f is None else C.byref(f), _ptr(t_at), _ptr(out.get('iter_max')), C.byref(g)))
        elif f is None:
            _check(self.lib.d2d_sim_track_run(*args))
        elif t_at is not None:
            _check(self.lib.d2d_sim_track_run_wind_at(*args, C.byref(f), _ptr(t_at), _ptr(out['iter_max'])))
        else:
            _check(self.lib.d2d_sim_track_run_wind(*args, C.byref(f), float(t_start), _ptr(out['iter_max'])))
        return out

    def _constraint_rows(self, rows, n, width, cap, what):
        """A per-drone constraint table for track_dispersion -> a contiguous device tensor [n][k][width] or None.  rows: None, an
        object with lowered() (d2d.opty_utils.GeoFence: the same rows for every drone), an array (k, width) shared by every drone, or
        an array / device tensor [n][k][width]."""
        torch = _torch()
        if rows is None:
            return None
        if hasattr(rows, 'lowered'):
            rows = rows.lowered()
        if not hasattr(rows, 'data_ptr'):
            rows = np.asarray(rows, dtype=np.float64)
            if rows.ndim == 2:
                rows = np.broadcast_to(rows[None], (n,) + rows.shape)
            rows = self.dev(np.ascontiguousarray(rows))
        if rows.dim() != 3 or rows.shape[0] != n or rows.shape[2] != width or rows.dtype != torch.float64 or rows.device.type != 'cuda':
            raise ValueError(f'{what}: rows [{n}][k][{width}] of float64 on the device are required, got {tuple(rows.shape)} {rows.dtype}')
        if not 1 <= rows.shape[1] <= cap:
            raise ValueError(f'{what}: 1 .. {cap} rows per drone, got {rows.shape[1]}')
        return rows.contiguous()

    def track_dispersion(self, x_ref, y_ref, w=(0.0, 0.0), gust=None, time=None, dt=None, fence=None, keep_out=None, S0=None, record_P=False,
                         **kw):
        """The gust dispersion of tracked plans (d2d_track_dispersion): the covariance of the deviation of track_run(gust=...) from the
        gust-free flight of the same references, by one deterministic pass per plan.  x_ref, y_ref dev [T][n] as track_run takes them;
        time (its first two entries give the step) or dt; w: the constant wind handed to the controller and the plant; gust: a
        d2d.wind.GustModel (only sigma and tau enter: the prediction is per aircraft, see full_sim.dispersion_margin for pairs).
        fence: a d2d.opty_utils.GeoFence, lowered rows (k, 4), or rows per drone [n][k][4]; keep_out: discs (k, 3) = (cx, cy, R) or
        [n][k][3].  S0 dev [28][n]: the packed covariance to start from (S_out of an earlier call), None: no tracking error and the
        stationary gust.  kw: track_params' controller constants (tau_phi, tau_v, Q, R, ...).
        Returns a dict of device tensors: S [28][n], sig_max, sig_row [n], with record_P Ppos [T][3][n] (xx, xy, yy), with a fence
        fence_sn, fence_k, fence_row [k][n], with discs disc_k, disc_row [k][n]."""
        if not hasattr(gust, 'numbers'):
            raise TypeError(f'{type(gust).__name__} is not a gust model: build one with d2d.wind.GustModel')
        if (time is None) == (dt is None):
            raise ValueError('give the time grid as time= or its step as dt=, not both')
        torch = _torch()
        if dt is None:
            dt = float(time[1] - time[0])
        T, n = x_ref.shape
        assert y_ref.shape == x_ref.shape and x_ref.is_contiguous() and y_ref.is_contiguous() and x_ref.dtype == y_ref.dtype == torch.float64
        p = self.track_params(n, T, float(dt), w=(float(w[0]), float(w[1])), **kw)
        k = gust.numbers(float(dt))
        if S0 is not None:
            assert S0.is_contiguous() and tuple(S0.shape) == (28, n) and S0.dtype == torch.float64 and S0.device.type == 'cuda'
        din = DispersionIn(k['a'], k['s'], k['sigma'], None if S0 is None else S0.data_ptr())
        edges = self._constraint_rows(fence, n, 4, MAX_FENCE, 'track_dispersion: fence')
        discs = self._constraint_rows(keep_out, n, 3, MAX_KEEP, 'track_dispersion: keep_out')
        i32 = torch.int32
        out = dict(S=self.empty(28, n), sig_max=self.empty(n), sig_row=self.empty(n, dtype=i32))
        if record_P:
            out['Ppos'] = self.empty(T, 3, n)
        if edges is not None:
            ne = edges.shape[1]
            out.update(fence_sn=self.empty(ne, n), fence_k=self.empty(ne, n), fence_row=self.empty(ne, n, dtype=i32))
        if discs is not None:
            out.update(disc_k=self.empty(discs.shape[1], n), disc_row=self.empty(discs.shape[1], n, dtype=i32))
        names = dict(Ppos_hist='Ppos', S_out='S')
        dout = DispersionOut(*[None if out.get(names.get(f, f)) is None else out[names.get(f, f)].data_ptr() for f in DISPERSION_OUT])
        fc = None if edges is None else FenceC(edges.shape[1], 0, edges.data_ptr())
        kc = None if discs is None else KeepOutC(discs.shape[1], 0, discs.data_ptr())
        _check(self.lib.d2d_track_dispersion(self.h, C.byref(p), _ptr(x_ref), _ptr(y_ref), C.byref(din), None if fc is None else C.byref(fc),
                                             None if kc is None else C.byref(kc), C.byref(dout)))
        return out                                    # (edges, discs are released here: the context's stream is torch's, whose allocator orders reuse)


_default_ctx = None


def default_context():
    """Process-wide context on cuda:LOCAL_RANK used by the reference-named mirror classes."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get('LOCAL_RANK', 0)))
    return _default_ctx


class FitPlan:
    """Shared basis block + solver scratch for one (S, K, duration, wref)."""

    def __init__(self, ctx, S, K, duration, wref, kernel='auto', long_tables=-1):
        """kernel: 'auto' | 'knot' | 'fused' | 'long' | 'split' (d2d_fit_plan_opts.kernel: which kernel family serves d2d_fit_solve);
        long_tables: d2d_fit_plan_opts.long_tables (-1 = the segment formulation)."""
        self.ctx, self.S, self.K, self.duration = ctx, S, K, float(duration)
        self.nq = 4 * S
        w = np.ascontiguousarray(wref, dtype=np.float64)
        h = _P()
        po = FitPlanOpts(KERNELS[kernel], int(long_tables), (C.c_int32 * 2)(0, 0))
        _check(ctx.lib.d2d_fit_plan_create_ex(ctx.h, S, K, self.duration, _hptr(w), C.byref(po), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            self.ctx.lib.d2d_fit_plan_destroy(self.h)
            self.h = None

    __del__ = close

    @property
    def kernel(self):
        """'fused' | 'long' | 'split' | 'knot': the kernel d2d_fit_solve runs for this plan with the default solver (include/d2d.h
        D2D_FIT_KERNEL_*; 'knot' = the fused shape in knot coordinates, csrc/fit_knot.hip)."""
        return ('split', 'fused', 'long', 'knot')[self.ctx.lib.d2d_fit_plan_kernel(self.h)]

    def basis(self):
        """Host copies: G (3,K,nq), Gp (3,K,4), Z (8S,nq), Zp (8S,4), Pinit (nq,K)."""
        S, K, nq = self.S, self.K, self.nq
        G = np.empty((3, K, nq)); Gp = np.empty((3, K, 4)); Z = np.empty((8 * S, nq)); Zp = np.empty((8 * S, 4))
        P = np.empty((nq, K))
        _check(self.ctx.lib.d2d_fit_plan_get(self.h, _hptr(G), _hptr(Gp), _hptr(Z), _hptr(Zp), _hptr(P)))
        return G, Gp, Z, Zp, P

    def init(self, scen):
        B = scen.shape[0]
        q = self.ctx.empty(B, 2 * self.nq)
        _check(self.ctx.lib.d2d_fit_init(self.ctx.h, self.h, B, _ptr(scen), _ptr(q)))
        return q

    def project(self, scen, xy):
        """xy dev [B][2][K] node positions -> q0 dev [B][2nq]."""
        B = scen.shape[0]
        q = self.ctx.empty(B, 2 * self.nq)
        _check(self.ctx.lib.d2d_fit_project(self.ctx.h, self.h, B, _ptr(scen), _ptr(xy), _ptr(q)))
        return q

    def eval(self, scen, q, want_H=True):
        torch = _torch()
        B, n = scen.shape[0], 2 * self.nq
        cost, g = self.ctx.empty(B), self.ctx.empty(B, n)
        H = torch.zeros(B, n, n, dtype=torch.float32, device=self.ctx.device) if want_H else None
        _check(self.ctx.lib.d2d_fit_eval(self.ctx.h, self.h, B, _ptr(scen), _ptr(q), _ptr(cost), _ptr(g), _ptr(H)))
        return cost, g, H

    def solve(self, scen, q, max_iter=200, check_every=8, ftol=1e-14, gtol=1e-9, xtol=1e-11, so_lambda=SO_LAMBDA, **mode_kw):
        """In-place LM solve of q.  Returns cost, iters, status (device) and stats (numpy[4]).
        mode_kw: mode (MODE_MINPACK default / MODE_FAST), mp_finish, mp_tol, slice (fit_opts)."""
        torch = _torch()
        B = scen.shape[0]
        cost = self.ctx.empty(B)
        iters = torch.empty(B, dtype=torch.int32, device=self.ctx.device)
        status = torch.empty(B, dtype=torch.int32, device=self.ctx.device)
        stats = np.zeros(4)
        o = fit_opts(max_iter, check_every, ftol, gtol, xtol, so_lambda, **mode_kw)
        _check(self.ctx.lib.d2d_fit_solve(self.ctx.h, self.h, B, _ptr(scen), _ptr(q), C.byref(o), _ptr(cost),
                                          _ptr(iters), _ptr(status), _hptr(stats)))
        return cost, iters, status, stats

    # -- the same loop in parts (for a caller-side / cross-GPU convergence check) -------
    def begin(self, B):
        _check(self.ctx.lib.d2d_fit_begin(self.ctx.h, self.h, B))

    def iterate(self, scen, q, n_iters, max_iter=200, ftol=1e-14, gtol=1e-9, xtol=1e-11, so_lambda=SO_LAMBDA, **mode_kw):
        """Run n_iters more damped solves; returns the number of trajectories still running."""
        o = fit_opts(max_iter, n_iters, ftol, gtol, xtol, so_lambda, **mode_kw)
        running = C.c_int32(0)
        _check(self.ctx.lib.d2d_fit_iterate(self.ctx.h, self.h, scen.shape[0], _ptr(scen), _ptr(q), C.byref(o), n_iters,
                                            C.byref(running)))
        return running.value

    def finish(self, scen, q):
        torch = _torch()
        B = scen.shape[0]
        cost = self.ctx.empty(B)
        iters = torch.empty(B, dtype=torch.int32, device=self.ctx.device)
        status = torch.empty(B, dtype=torch.int32, device=self.ctx.device)
        stats = np.zeros(4)
        _check(self.ctx.lib.d2d_fit_finish(self.ctx.h, self.h, B, _ptr(scen), _ptr(q), _ptr(cost), _ptr(iters),
                                           _ptr(status), _hptr(stats)))
        return cost, iters, status, stats

    def order_from_iters(self, iters):
        """Scheduling hint: hand the fits of the next solves of this batch out longest-first (iters: device int32 [B] of a
        previous solve of the same scenarios)."""
        _check(self.ctx.lib.d2d_fit_plan_set_order(self.ctx.h, self.h, iters.shape[0], _ptr(iters)))

    def clear_order(self):
        _check(self.ctx.lib.d2d_fit_plan_set_order(self.ctx.h, self.h, 0, None))

    def set_handout_prior(self, table=None):
        """Install a hand-out prior (float32 [2][48][12] expected trial counts, d2dhip.handout.fit_prior) or, with None, the built-in one."""
        t = None if table is None else np.ascontiguousarray(table, dtype=np.float32).reshape(2, 48, 12)
        _check(self.ctx.lib.d2d_fit_plan_set_handout_prior(self.ctx.h, self.h, _hptr(t)))

    def learn_handout_prior(self, scen, iters):
        """Calibrate the prior on a finished solve of this workload: scen [B][SCEN_STRIDE], iters [B] (device or host)."""
        from . import handout
        sc = scen.cpu().numpy() if hasattr(scen, 'cpu') else np.asarray(scen)
        it = iters.cpu().numpy() if hasattr(iters, 'cpu') else np.asarray(iters)
        table = handout.fit_prior(sc, self.duration, it)
        self.set_handout_prior(table)
        return table

    def last_order(self, B):
        """The hand-out order the last solve launch used (int32 [B]); raises if it ran in index order."""
        o = np.zeros(B, np.int32)
        _check(self.ctx.lib.d2d_fit_plan_get_order(self.ctx.h, self.h, B, _hptr(o)))
        return o

    def group_order_from_last(self, R, enable=True):
        """Scheduling hint for solve_groups over R scenarios: start the scenarios that swept longest in the LAST solve_groups
        of this plan first (enable=False clears it)."""
        _check(self.ctx.lib.d2d_fit_plan_set_group_order(self.ctx.h, self.h, R, 1 if enable else 0))

    def group_report(self, R):
        """(sweeps int32 [R], last-sweep largest relative move float64 [R]) of the last solve_groups over R scenarios.
        A refused scenario (a first evaluation that is not finite: include/d2d.h d2d_fit_group_report) reports 0 sweeps and a NaN move."""
        sw = np.zeros(R, np.int32); mv = np.zeros(R)
        _check(self.ctx.lib.d2d_fit_group_report(self.ctx.h, self.h, R, _hptr(sw), _hptr(mv)))
        return sw, mv

    def set_groups(self, n_ac):
        _check(self.ctx.lib.d2d_fit_plan_set_groups(self.h, n_ac))
        self.n_group = n_ac

    def solve_groups(self, scen, q, n_ac, max_sweeps=60, inner_iters=8, tol=1e-12, ftol=1e-14, gtol=1e-9, xtol=1e-11, **gs_kw):
        """Block Gauss-Seidel over the aircraft of every group (scen / q rows g*n_ac + i).  Returns the
        per-aircraft sub-problem costs (device), sweeps used and stats (numpy[4])."""
        if getattr(self, 'n_group', 1) != n_ac:
            self.set_groups(n_ac)
        B = scen.shape[0]
        assert B % n_ac == 0
        cost = self.ctx.empty(B)
        o = fit_opts(inner_iters, 1, ftol, gtol, xtol, 0.0, **gs_kw)      # gs_kw: gs_ls, gs_ls_s0, gs_ls_r0, gs_prio_at, gs_pairs
        sw = C.c_int32(0)
        stats = np.zeros(4)
        _check(self.ctx.lib.d2d_fit_solve_groups(self.ctx.h, self.h, B // n_ac, _ptr(scen), _ptr(q), C.byref(o), max_sweeps,
                                                 inner_iters, tol, _ptr(cost), C.byref(sw), _hptr(stats)))
        return cost, sw.value, stats

    def profile(self, enable):
        _check(self.ctx.lib.d2d_fit_profile(self.h, 1 if enable else 0))

    def rows(self, scen, q):
        """Residual rows at q: cost, J^T r (device); the fp32 row records stay in the plan's scratch for jtj()."""
        B, n = scen.shape[0], 2 * self.nq
        cost, g = self.ctx.empty(B), self.ctx.empty(B, n)
        _check(self.ctx.lib.d2d_fit_rows(self.ctx.h, self.h, B, _ptr(scen), _ptr(q), _ptr(cost), _ptr(g)))
        return cost, g

    def jtj(self, B, want_H=True):
        """J^T J from the records of the last rows(): the contraction-only launch.  H dev [B][2nq][2nq] or None."""
        torch = _torch()
        n = 2 * self.nq
        H = torch.zeros(B, n, n, dtype=torch.float32, device=self.ctx.device) if want_H else None
        _check(self.ctx.lib.d2d_fit_jtj(self.ctx.h, self.h, B, _ptr(H)))
        return H

    def profile_read(self):
        """(eval_ms, eval_launches, step_ms, step_launches, fused_lm_ms, fused_lm_launches, jtj_ms, jtj_launches) from HIP
        events."""
        out = np.zeros(8)
        _check(self.ctx.lib.d2d_fit_profile_read(self.h, _hptr(out)))
        return out

    def coeffs(self, scen, q):
        B = scen.shape[0]
        z = self.ctx.empty(B, 2, self.S, 8)
        _check(self.ctx.lib.d2d_fit_coeffs(self.ctx.h, self.h, B, _ptr(scen), _ptr(q), _ptr(z)))
        return z

    def sample(self, scen, q):
        B = scen.shape[0]
        Y, Xs = self.ctx.empty(B, 6, self.K), self.ctx.empty(B, 5, self.K)
        _check(self.ctx.lib.d2d_fit_sample(self.ctx.h, self.h, B, _ptr(scen), _ptr(q), _ptr(Y), _ptr(Xs)))
        return Y, Xs
