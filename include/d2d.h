/*
 * libd2dhip.so -- C ABI of the MI355X (gfx950) batched trajectory-fit and
 * guidance-simulation engine.
 *
 * The reference (rajashree-srikanth/drone-sim-python) is pure Python and has no FFI; each
 * entry point below names the Python interface it replaces (file:line relative to the
 * reference's repository root) and is what a ctypes binding on the reference side would
 * bind (INTEGRATION.md shows the stubs).
 *
 * Conventions
 *   - every function returns 0 on success or a negative D2D_E* code; d2d_last_error()
 *     returns a thread-local message for the last failure.  No exception crosses the ABI.
 *   - "dev" pointers are device (HBM) addresses owned by the caller (e.g.
 *     torch.Tensor.data_ptr() of a contiguous ROCm tensor); "host" pointers are ordinary
 *     host memory.  The library allocates only scratch tied to a context or a fit plan.
 *   - all work is enqueued on the hipStream_t given to d2d_ctx_create and is asynchronous
 *     unless stated; the caller synchronises the stream.
 *   - one context per GPU per host thread; calls are re-entrant across contexts.
 *   - device arrays are "plane-major" (structure of arrays): a state history is
 *     [row][component][drone] so that one wavefront writes 64 consecutive doubles.
 */
#ifndef D2D_H
#define D2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_VERSION 129

/* error codes */
#define D2D_OK 0
#define D2D_EINVAL (-1)   /* bad argument (shape, null pointer, unsupported size) */
#define D2D_EHIP (-2)     /* a HIP runtime call failed */
#define D2D_ENOMEM (-3)
#define D2D_ESTATE (-4)   /* call order / plan mismatch */

typedef struct d2d_ctx d2d_ctx;
typedef struct d2d_fit_plan d2d_fit_plan;

int d2d_version(void);
const char *d2d_last_error(void);

/* device = HIP device ordinal; stream = hipStream_t (NULL = the default stream). */
int d2d_ctx_create(int device, void *stream, d2d_ctx **out);
int d2d_ctx_destroy(d2d_ctx *ctx);
int d2d_ctx_sync(d2d_ctx *ctx);   /* hipStreamSynchronize on the context's stream */

/* Multi-GPU convergence exchange (one process per GPU; BASELINE configs[3]: trajectories shard by rank, the only collective is this
 * one).  The reference has no counterpart (it is single-process Python); SURVEY.md 8b asks for the entry point so that a host
 * without torch.distributed can drive the sharded solve.  RCCL is loaded at run time (dlopen of librccl.so.1): the library has
 * no link-time dependency on it.
 *   d2d_comm_available  local, no communication: D2D_OK when this process can load RCCL and resolve the symbols used below.
 *                       d2d_comm_create is itself a collective (ncclCommInitRank returns when ALL ranks have joined): a host
 *                       agrees on this flag over its own channel first and calls d2d_comm_create only if every rank reported
 *                       D2D_OK -- a rank that cannot get there would leave the others waiting inside it;
 *   d2d_comm_unique_id  rank 0 creates the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by whatever channel the
 *                       host has (a file, MPI, a TCP store);
 *   d2d_comm_create     every rank, same id: ncclCommInitRank on the context's device;
 *   d2d_allreduce_stats stats dev double[3] in place, enqueued on the context's stream as ONE grouped exchange:
 *                       [0] sum (cost), [1] max (|J^T r|_inf), [2] sum (trajectories neither converged nor stalled) -- the three scalars
 *                       d2d_fit_finish reports in stats[0..2].  The caller synchronises the stream before reading them. */
typedef struct d2d_comm d2d_comm;
#define D2D_COMM_ID_BYTES 128
int d2d_comm_available(void);
int d2d_comm_unique_id(void *id_out);
int d2d_comm_create(d2d_ctx *ctx, const void *id, int rank, int world, d2d_comm **out);
int d2d_comm_destroy(d2d_comm *comm);
int d2d_comm_info(const d2d_comm *comm, int32_t *rank, int32_t *world);   /* ncclCommUserRank / ncclCommCount of the communicator (either may be NULL); D2D_ESTATE if they differ from what d2d_comm_create was given */
int d2d_allreduce_stats(d2d_ctx *ctx, d2d_comm *comm, double *stats);     /* D2D_EINVAL if stats is not device memory */

/* ------------------------------------------------------------------------------------
 * Plant and guidance (fp64).  State components: x, y, psi, phi, v; inputs: phi_c, v_c.
 * ------------------------------------------------------------------------------------ */

/* Gauss-Legendre Runge-Kutta quadrature of the plant step: D2D_GL_PANELS panels on
 * dt*[edge_p, edge_p+1], D2D_GL_STAGES stages each; phi and v (first-order lags under
 * a zero-order-hold input) are integrated exactly. */
#define D2D_GL_STAGES 4
#define D2D_GL_PANELS 5
/* ... and a step that starts within D2D_GL_FAST_DPHI (rad) of its bank command -- every step of a settled guidance loop -- takes ONE
 * panel of D2D_GL_FAST_STAGES stages over the whole step instead (the boundary layer it has to resolve is that small) */
#define D2D_GL_FAST_STAGES 6
#define D2D_GL_FAST_DPHI 0.02
#define D2D_GL_FAST_RATIO 6.0      /* ... and only while dt <= GL_FAST_RATIO * tau_phi: the one panel integrates exp(-t / tau_phi) over the whole step
                                      (error at the threshold: 2e-10 at dt = 5 tau_phi, 7e-8 at 10 tau_phi, 8e-6 at 20 tau_phi; the graded panels: <= 1e-9) */

/* One batched plant step.  Replaces Aircraft.disc_dyn(Xk, Uk, W, t, dt)
 * (src/d2d/dynamic.py:25-28; model :14-23, heading wrap :27 / src/d2d/utils.py:7).
 * X, Xout: dev [5][n]; U: dev [2][n]; wind (wx, wy) constant. */
int d2d_step(d2d_ctx *ctx, int n, const double *X, const double *U, double wx, double wy,
             double tau_phi, double tau_v, double dt, double *Xout);

typedef struct {
  int32_t n_form;      /* independent formations                                   */
  int32_t n_ac;        /* aircraft per formation, 1..64                            */
  int32_t n_rows;      /* rows of the time grid, len(arange(t_start,t_end,t_step)) */
  int32_t rec_stride;  /* history rows are kept for i % rec_stride == 0 (>=1)      */
  double dt, tau_phi, tau_v;
  double ke, kd, kr;   /* GVF / DCF gains (src/11_full_sim_case1.py:108-110)       */
  double v_c;          /* commanded airspeed (the `v` argument, :93)               */
  double wx, wy;       /* wind                                                     */
  int32_t use_stop;    /* 1: the state rule of case 1 (:140,170-175): every aircraft within stop_tol of X0f;
                          2: the phase-error rule of cases 2 / 3 (src/12_full_sim_case2.py:156-164,
                          src/12_full_sim_case3.py:163-178): every inter-vehicle phase error (degrees,
                          signed) <= stop_tol[0]                                      */
  int32_t stop_hold;   /* rule 2: the loop goes on for this many further steps on which the rule holds
                          (case 3 waits t_opt_comp = 0.7 s for the planner: 14 steps); 0 = case 2 */
  double stop_tol[3];  /* rule 1: |x|,|y|,|psi| tolerances, reference: 3, 3, 0.5 deg; rule 2: [0] = degrees */
} d2d_gvf_params;

/* Circular-formation phase: DCF phase consensus + GVF circle following + plant step, the
 * whole time loop on the device.  Replaces CircularFormationGVF(c, r, v, n_ac, X0f, ...)
 * (src/11_full_sim_case1.py:93-177; identical loop src/09_CircularFormation_diffcentre.py
 * :91-115) and the per-step calls it makes: DCFController.get (src/d2d/guidance.py:103-126),
 * CircleTraj.get (:137-146), GVFcontroller.get (:155-181), atan(U/9.81) (11_*:160),
 * Aircraft.disc_dyn (src/d2d/dynamic.py:25-28).
 * N = n_form*n_ac drones, drone d = formation d/n_ac, aircraft d%n_ac.
 *   X0       dev [5][N]   initial states (row 0 of the history)
 *   centres  dev [2][N]   circle centre of each drone
 *   radius   dev [N]      nominal radius r
 *   Bmat     host [n_ac][n_ac-1] incidence matrix (ConstructBMatrix, 11_*:81-91)
 *   z_des    host [n_ac-1] desired inter-vehicle angles
 *   X0f      dev [3][N] or NULL: x,y,psi targets of the stop rule
 *   X_hist   dev [n_rec][5][N] or NULL; U_hist dev [n_rec][2][N] or NULL (row i-1 holds the
 *            input applied during step i, as the reference writes U_array[i-1]);
 *   Rr_hist  dev [n_rec][N] or NULL (commanded radius, row i); eth_hist dev
 *            [n_rec][n_form*(n_ac-1)] or NULL (phase errors in degrees, row i)
 *            with n_rec = ceil(n_rows / rec_stride)
 *   X_final  dev [5][N]: state after the last executed step
 *   stop_row dev int32 [n_form]: rows kept by the reference's trim when its `break` fires (rule 1 breaks at the top of
 *            step i: i rows; rule 2 at the end of step i: i + 1 rows), or n_rows if the rule never fired;
 *   conv_row dev int32 [n_form] or NULL: rule 2, the reference's `index` = i - 1 of the first step on which the rule held
 *            (-1: never).
 * A formation that has stopped is frozen (its rows beyond stop_row are not written). */
int d2d_sim_gvf_run(d2d_ctx *ctx, const d2d_gvf_params *p, const double *X0,
                    const double *centres, const double *radius, const double *Bmat,
                    const double *z_des, const double *X0f, double *X_hist, double *U_hist,
                    double *Rr_hist, double *eth_hist, double *X_final, int32_t *stop_row, int32_t *conv_row);

typedef struct {
  int32_t n;           /* drones (independent)                                     */
  int32_t n_rows;      /* rows of the reference time grid                          */
  double dt, tau_phi, tau_v;
  double wx, wy;       /* wind handed to DiffController(w) and to the plant        */
  double err_sats[5];  /* src/Controllers.py:147                                   */
  double v_min, v_max, phi_lim;        /* :148-149                                 */
  double q_diag[5], r_diag[2];         /* :152                                     */
} d2d_track_params;

/* One batched evaluation of DiffController.ComputeGain (src/Controllers.py:159-186):
 * ComputeFlatness (:62-108), error wrap/clip (:165-169), Aircraft.cont_jac
 * (src/d2d/dynamic.py:32-43), control.lqr (:174; 5x5 continuous algebraic Riccati
 * equation solved on the device), U = clip(Ur - K dX) (:183-185).
 *   X dev [5][n]; Yref dev [8][n] = x,y,xd,yd,xdd,ydd,xddd,yddd
 *   outputs (dev, any may be NULL): Xr [5][n], dX [5][n], U [2][n], Kgain [10][n]
 *   (K row-major 2x5 per drone, plane-major across drones). */
int d2d_ctrl_gain(d2d_ctx *ctx, const d2d_track_params *p, const double *X, const double *Yref,
                  double *Xr, double *dX, double *U, double *Kgain);

/* One batched evaluation of the legacy DFFFController.get(X, t) (src/d2d/guidance.py:62-91):
 * DiffFlatness.state_and_input_from_output (:22-47) of the reference sample, error wrap (psi) and clip
 * (:70-72), Aircraft.cont_jac, control.lqr on the 3-state sub-system A[:3,:3], A[:3,3:] (:78-81; 3x3
 * Riccati equation solved on the device), U = clip(Ur - K dX) (:85-88).  Of d2d_track_params it reads n,
 * tau_phi, tau_v, wx, wy, err_sats, q_diag[0..2], r_diag, phi_lim, v_min, v_max.
 *   X dev [5][n]; Yref dev [6][n] = x,y,xd,yd,xdd,ydd (the sample traj.get(t) of every drone)
 *   outputs (dev, any may be NULL): Xr [5][n], U [2][n], Kgain [6][n] (K1 row-major 2x3; the phi and v
 *   columns of the reference's 2x5 K are zero). */
int d2d_dfff_eval(d2d_ctx *ctx, const d2d_track_params *p, const double *X, const double *Yref,
                  double *Xr, double *U, double *Kgain);

/* Trajectory-tracking phase, whole time loop on the device.  Replaces
 * implement_controller(n_ac, time, x_ref, y_ref, v, w, X0s)
 * (src/11_full_sim_case1.py:241-291) including ComputeDerivatives (:197-204; two passes
 * of numpy.gradient(edge_order=2)/dt per axis).
 *   x_ref, y_ref dev [n_rows][n]; X0 dev [5][n]
 *   X_hist dev [n_rows][5][n]; U_hist [n_rows][2][n]; Xr_hist, dX_hist [n_rows][5][n];
 *   Yd_hist, Ydd_hist [n_rows][2][n] (any history may be NULL); X_final dev [5][n].
 * Row conventions as the reference: step i uses reference sample i and state i-1 and
 * writes U, dX, Xr, Yd, Ydd at row i-1 and X at row i. */
int d2d_sim_track_run(d2d_ctx *ctx, const d2d_track_params *p, const double *x_ref,
                      const double *y_ref, const double *X0, double *X_hist, double *U_hist,
                      double *Xr_hist, double *dX_hist, double *Yd_hist, double *Ydd_hist,
                      double *X_final);

/* The legacy simulation loop run_simulation(time, aircraft, windfield, ctl, X0, perts)
 * (src/05_test_simulation.py:21-34) with DFFFController (src/d2d/guidance.py:52-91) for n independent aircraft:
 *   U[i-1] = ctl.get(X[i-1], t[i-1]); X[i] = disc_dyn(X[i-1], U[i-1], w, t[i-1], dt) + perts[i]; U[T-1] = ctl.get(X[T-1]).
 *   Yref dev [n_rows][6][n]: the trajectory's flat outputs at the sample times (x, y, xd, yd, xdd, ydd: what
 *   traj.get(t) returns, without the jerk the controller never reads); perts dev [n_rows][5][n] or NULL;
 *   X0 dev [5][n]; X_hist dev [n_rows][5][n], U_hist [n_rows][2][n], Xr_hist [n_rows][5][n] (any may be NULL);
 *   X_final dev [5][n] or NULL.  Controller constants as d2d_dfff_eval (p->q_diag[0..2], r_diag, err_sats, limits). */
int d2d_sim_dfff_run(d2d_ctx *ctx, const d2d_track_params *p, const double *Yref, const double *perts,
                     const double *X0, double *X_hist, double *U_hist, double *Xr_hist, double *X_final);

/* Reference trajectories of the legacy simulations, sampled on the device: Yref [T][6][n] (x, y, xd, yd, xdd, ydd at
 * t_start + i dt) -- the input of d2d_sim_dfff_run -- for n trajectories described by desc dev [n][D2D_TRAJ_STRIDE]:
 *   desc[0] = number of segments (1..D2D_TRAJ_MAX_SEG), desc[1] = the composite's t0, desc[2] = its total duration,
 *   desc[3] = 1: periodic composite (CompositeTraj.get, src/d2d/trajectory.py:202-208: fmod(t - t0, duration), first segment
 *   whose cumulative end is beyond the lapse) / 0: one plain segment evaluated at t;
 *   then per segment D2D_TRAJ_SEG_STRIDE doubles: type, the segment's t0, its cumulative end, parameters:
 *     D2D_TRAJ_LINE    p1x, p1y, unx, uny, v                      TrajectoryLine (src/d2d/trajectory.py:125-141)
 *     D2D_TRAJ_CIRCLE  cx, cy, r, omega = v/r, alpha0             TrajectoryCircle (:143-160)
 *     D2D_TRAJ_SLALOM  p1x, p1y, unx, uny, v, a, om, phi          TrajSlalom (src/d2d/trajectory_factory.py:113-137)
 *     D2D_TRAJ_POLY    coefs[0,:] of the x polynomial (8), of y (8)  MinSnapPoly (src/d2d/trajectory.py:166-187)
 * (d2d/trajectory.py `describe` builds these rows from the mirrored trajectory classes). */
#define D2D_TRAJ_MAX_SEG 8
#define D2D_TRAJ_SEG_STRIDE 20
#define D2D_TRAJ_STRIDE (4 + D2D_TRAJ_MAX_SEG * D2D_TRAJ_SEG_STRIDE)
enum { D2D_TRAJ_LINE = 1, D2D_TRAJ_CIRCLE = 2, D2D_TRAJ_SLALOM = 3, D2D_TRAJ_POLY = 4 };
int d2d_traj_sample(d2d_ctx *ctx, int n, int T, double t_start, double dt, const double *desc, double *Yref);

/* Wind fields that vary in space and time: the plug-point WindField.sample(t, loc) of the reference's plant
 * (src/d2d/dynamic.py:14-16, 25-28: the field at the aircraft's own position and time, on every right-hand-side evaluation).
 * A field is a uniform tensor-product cubic B-spline (C2, so the Gauss panels keep their order) over (x, y) -- steady, nt = 1 --
 * or over (t, x, y) -- unsteady, nt >= 4.  Along an axis with n control points, first knot u0 and spacing h the spline lives on
 * [u0, u0 + (n - 3) h]: s = (u - u0) / h, segment i = min(floor(s), n - 4), r = s - i, and the value is
 * sum_k B_k(r) c[i + k] with the uniform cubic B-spline weights B_0 = (1-r)^3/6, B_1 = (3r^3 - 6r^2 + 4)/6,
 * B_2 = (-3r^3 + 3r^2 + 3r + 1)/6, B_3 = r^3/6.  A query outside the box is clamped to it coordinate by coordinate: the field is
 * held at its boundary value there, which is continuous but only C0 across the boundary.
 *   cp dev [nt][2][ny][nx]: control points, component 0 = wx, 1 = wy (the two components of a point share 128-byte lines).
 * nx, ny < 4, nt not in {1} or [4, inf), hx, hy (and ht when nt > 1) not > 0, or cp NULL: D2D_EINVAL.  (version 111) */
typedef struct {
  int32_t nt, ny, nx;      /* control points per axis; nt = 1: steady (2-D spline), else nt >= 4 */
  int32_t pad;
  double t0, ht;           /* first knot and knot spacing in t (ignored when nt = 1) */
  double x0, hx, y0, hy;   /* same in x, y */
  const double *cp;        /* dev [nt][2][ny][nx] control points (component 0 = wx, 1 = wy) */
} d2d_wind_field;

/* In a field the stage positions of a Gauss panel are implicit: x_i = x + w sum_j A_ij (v_j cos psi_j + wx(t + c_j w, x_j, y_j)),
 * the same for y (phi, v and the heading stay exact / explicit as in d2d_step).  They are solved by fixed-point iteration on the
 * wind term, started from the field at the panel's start, until the largest update of a stage position over the wavefront is
 * <= D2D_WIND_TOL (1 + |x|) (resp. |y|), or D2D_WIND_MAX_ITERS field sweeps; the panel's end takes the converged stage winds.
 * iter_max (dev int32 [1] or NULL): the largest number of sweeps any stage solve of the call used. */
#define D2D_WIND_TOL 1e-13
#define D2D_WIND_MAX_ITERS 8

/* Batched evaluation of a field: t dev [n], xy dev [2][n], w dev [2][n] (wx, wy). */
int d2d_wind_sample(d2d_ctx *ctx, const d2d_wind_field *f, int n, const double *t, const double *xy, double *w);

/* d2d_step in a field: the step starts at time t. */
int d2d_step_wind(d2d_ctx *ctx, int n, const double *X, const double *U, double t, const d2d_wind_field *f, double tau_phi,
                  double tau_v, double dt, double *Xout, int32_t *iter_max);

/* The three time loops in a field.  Same arguments as their twins, plus the field, the time of row 0 (row i is at
 * t_start + i dt, as np.arange makes it) and iter_max.  The plant flies the field; what the controller sees follows the reference:
 *   d2d_sim_gvf_run_wind    no wind (GVFcontroller stores it and never reads it, src/d2d/guidance.py:149-181); p->wx, p->wy are
 *                           not used.  Every formation size takes the general (LDS-exchange) kernel;
 *   d2d_sim_track_run_wind  p->wx, p->wy: the constant of DiffController(w) (src/11_full_sim_case1.py:241-291 builds WindField(w)
 *                           for the plant and hands w to the controller separately);
 *   d2d_sim_dfff_run_wind   the field at (t_i, position of the reference sample i), as DFFFController.get samples it
 *                           (src/d2d/guidance.py:62-65); p->wx, p->wy are not used.
 * Wind derivatives stay zero in the flatness maps, as in the reference. */
int d2d_sim_gvf_run_wind(d2d_ctx *ctx, const d2d_gvf_params *p, const double *X0, const double *centres, const double *radius,
                         const double *Bmat, const double *z_des, const double *X0f, double *X_hist, double *U_hist, double *Rr_hist,
                         double *eth_hist, double *X_final, int32_t *stop_row, int32_t *conv_row, const d2d_wind_field *f,
                         double t_start, int32_t *iter_max);
int d2d_sim_track_run_wind(d2d_ctx *ctx, const d2d_track_params *p, const double *x_ref, const double *y_ref, const double *X0,
                           double *X_hist, double *U_hist, double *Xr_hist, double *dX_hist, double *Yd_hist, double *Ydd_hist,
                           double *X_final, const d2d_wind_field *f, double t_start, int32_t *iter_max);
int d2d_sim_dfff_run_wind(d2d_ctx *ctx, const d2d_track_params *p, const double *Yref, const double *perts, const double *X0,
                          double *X_hist, double *U_hist, double *Xr_hist, double *X_final, const d2d_wind_field *f, double t_start,
                          int32_t *iter_max);
/* d2d_sim_track_run_wind with a start time PER DRONE: t_start dev [n], drone j flies step i from t_start[j] + (i - 1) dt (the
 * drones of full_sim's mission chain start phase 2 at the row at which their own formation ended phase 1; the array is computed on
 * the device).  Same validation as d2d_sim_track_run_wind; t_start NULL: D2D_EINVAL.  With all entries equal to t0 the histories
 * are those of d2d_sim_track_run_wind(.., t0): the step's time is the same expression.  (version 113) */
int d2d_sim_track_run_wind_at(d2d_ctx *ctx, const d2d_track_params *p, const double *x_ref, const double *y_ref, const double *X0,
                              double *X_hist, double *U_hist, double *Xr_hist, double *dX_hist, double *Yd_hist, double *Ydd_hist,
                              double *X_final, const d2d_wind_field *f, const double *t_start, int32_t *iter_max);

/* Stochastic gusts: an unmeasured disturbance of the plant inside the time loops (version 118).  Each drone d flies, on top of the
 * constant wind or the field, the gust g = w_own o(d) + w_form h(formation of d): o is the drone's own process, h one process per
 * formation of n_ac consecutive drones (aircraft 50 m apart do not see independent air), w_own = sqrt(1 - c), w_form = sqrt(c) for a
 * formation correlation c in [0, 1).  The controllers never see it (the reference hands w to DiffController and WindField(w) to the
 * plant separately, src/11_full_sim_case1.py:241-291).
 *   Random numbers  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl increments 0x9E3779B9, 0xBB67AE85, ten rounds), one call
 *                   per process and step: counter = (step_base + step, stream & 0xffffffff, stream >> 32, sub), key = (seed &
 *                   0xffffffff, seed >> 32), sub = 2 phase + part (part 0: the drone's own process, 1: the formation's);
 *                   u1 = ((r0 >> 5) 2^26 + (r1 >> 6) + 0.5) 2^-53, u2 the same from r2, r3; (xi_x, xi_y) = sqrt(-2 ln u1) (cos, sin)(2 pi u2).
 *                   The own process of drone d draws on stream stream_base + d, the shared one on (stream_base + d) / n_ac: a gust is
 *                   a function of (seed, stream, phase, step) alone, bit for bit, whatever the batch, the block layout or the shard
 *                   (a shard passes the global index of its first drone as stream_base).
 *   Process         first-order Gauss-Markov per component, discretised exactly: o_i = a o_{i-1} + s xi_i, a = exp(-dt / tau),
 *                   s = sigma sqrt(1 - a^2), both computed by the host in fp64 (tau = L / V: the first-order Dryden form).  With
 *                   w_form = 0 the shared call is not made and the shared planes keep what they started with (0 without state_in).
 *   Time            a zero-order hold like the inputs: step i, from row i - 1 to row i, flies w + g_{i-1}; after the step the state
 *                   advances with the draw at counter step_base + i.  Every loop counts its steps from 1; `phase` separates the loops
 *                   of one mission (full_sim: phase 1 -> 0, phase 2 -> 1, repetition k of phase 3 -> 2 + k) and the state is handed
 *                   from loop to loop on the device.  step_base (0 in the loops of a mission) lets one series be CONTINUED under the
 *                   same phase word: a call from state_out with step_base advanced by the steps already made reproduces the rows
 *                   of one long call bit for bit.
 *   State           gs dev [4][N]: own x, own y, shared x, shared y (the shared planes replicated per aircraft).  state_in NULL: the
 *                   stationary start o_0 = sigma xi(step_base); given: o_0 is read from it and that draw is not made.  state_out (or
 *                   NULL): gs after the last EXECUTED step -- of a formation that stopped with stop_row = m, after step m - 1.
 *   g_hist          dev [n_rec][2][N] or NULL: row q holds g_q, the gust flown during step q + 1, on the rows X_hist keeps.
 * D2D_EINVAL before anything is launched: gust NULL; sigma or s negative or not finite; a outside [0, 1); a weight that is negative or
 * not finite, or w_own^2 + w_form^2 further than 1e-12 from 1; n_ac < 1, N % n_ac, stream_base % n_ac, stream_base < 0; phase or
 * step_base < 0, step_base + n_rows beyond the 32-bit step word.  n_ac is the gust's own (the tracking loop has none); in the
 * formation loop pass p->n_ac.  (phase is a non-negative int32, so sub = 2 phase + part < 2^32 never wraps: no two phases share
 * a word.)  A non-finite state_in entry is not detected, exactly as a non-finite X0 is not: it propagates as NaN into that drone's
 * gust, history and final state (shared planes: the caller keeps them equal within a formation). */
typedef struct {
  uint64_t seed;
  int64_t stream_base;     /* stream of drone 0 of this call: >= 0, a multiple of n_ac */
  int32_t phase;           /* >= 0: the loop of the mission */
  int32_t n_ac;            /* aircraft per formation: consecutive drones that share h */
  int64_t step_base;       /* added to the step counter; 0 unless a series is continued */
  double a, s, sigma;      /* exp(-dt / tau), sigma sqrt(1 - a^2), sigma (m/s) */
  double w_own, w_form;    /* sqrt(1 - c), sqrt(c) */
  const double *state_in;  /* dev [4][N] or NULL */
  double *state_out;       /* dev [4][N] or NULL */
  double *g_hist;          /* dev [n_rec][2][N] or NULL */
} d2d_gust;

/* The process alone, without a loop: rows 0 .. n_rows - 1 of g_hist [n_rows][2][N] and state_out after step n_rows - 1 -- the
 * statements of the time loops in the same order, so a loop's g equals this series bit for bit.  state_out and g_hist both NULL:
 * D2D_EINVAL. */
int d2d_gust_sample(d2d_ctx *ctx, int64_t N, int n_rows, const d2d_gust *gust);
/* d2d_sim_gvf_run / d2d_sim_gvf_run_wind through gusts: f NULL means the constant p->wx, p->wy (t_start, iter_max are then not used).
 * Every formation size takes the general (LDS-exchange) kernel.  A frozen formation does not advance its gust. */
int d2d_sim_gvf_run_gust(d2d_ctx *ctx, const d2d_gvf_params *p, const double *X0, const double *centres, const double *radius,
                         const double *Bmat, const double *z_des, const double *X0f, double *X_hist, double *U_hist, double *Rr_hist,
                         double *eth_hist, double *X_final, int32_t *stop_row, int32_t *conv_row, const d2d_wind_field *f,
                         double t_start, int32_t *iter_max, const d2d_gust *gust);
/* d2d_sim_track_run / _wind / _wind_at through gusts: f NULL means the constant p->wx, p->wy for the plant too; t_start dev [n] or
 * NULL (0 for every drone; not read without a field).  g_hist has n_rows rows. */
int d2d_sim_track_run_gust(d2d_ctx *ctx, const d2d_track_params *p, const double *x_ref, const double *y_ref, const double *X0,
                           double *X_hist, double *U_hist, double *Xr_hist, double *dX_hist, double *Yd_hist, double *Ydd_hist,
                           double *X_final, const d2d_wind_field *f, const double *t_start, int32_t *iter_max, const d2d_gust *gust);

/* Single batched evaluations behind the reference's per-call helper methods (the time
 * loops above fuse them; these exist so that host code written against the reference's
 * classes reaches the same device functions).
 *  d2d_dcf_eval : DCFController.get(n_ac, B, c, p, z_des, kr) (src/d2d/guidance.py:103-126);
 *                 centres, pos dev [2][N]; U_r dev [N]; eth_deg dev [n_form*(n_ac-1)] or NULL.
 *  d2d_gvf_eval : GVFcontroller.get(X, ke, kd, e, n, H) (:155-181); X dev [5][n], e dev [n],
 *                 nvec dev [2][n], H dev [4][n] (row-major 2x2); U dev [3][n] = U, U1, U2.
 *  d2d_flatness : variant 0 = DiffFlatness.state_and_input_from_output (:22-47),
 *                 variant 1 = DiffFlatness.ComputeFlatness (src/Controllers.py:62-108);
 *                 Yref dev [8][n]; X dev [5][n], U dev [2][n], Xdot dev [5][n] or NULL.
 *  d2d_cont_jac : Aircraft.cont_jac (src/d2d/dynamic.py:32-43); A dev [25][n], B dev [10][n].
 *  d2d_lqr      : control.lqr(A, B, Q, R) (call sites src/Controllers.py:174,
 *                 src/d2d/guidance.py:76,80) for 5-state / 2-input systems; Q host [25],
 *                 R host [4]; K dev [10][n], P dev [25][n] or NULL. */
int d2d_dcf_eval(d2d_ctx *ctx, int n_form, int n_ac, const double *Bmat, const double *z_des, double kr,
                 const double *centres, const double *pos, double *U_r, double *eth_deg);
int d2d_gvf_eval(d2d_ctx *ctx, int n, const double *X, const double *e, const double *nvec, const double *H,
                 double ke, double kd, double *U);
int d2d_flatness(d2d_ctx *ctx, int variant, int n, const double *Yref, double wx, double wy, double tau_phi,
                 double tau_v, double *X, double *U, double *Xdot);
int d2d_cont_jac(d2d_ctx *ctx, int n, const double *Xr, double tau_phi, double tau_v, double *A, double *B);
int d2d_lqr(d2d_ctx *ctx, int n, const double *A, const double *B, const double *Q, const double *R, double *K,
            double *P);

/* ------------------------------------------------------------------------------------
 * Polynomial trajectory fit: S segments x 2 axes x 8 monomial coefficients in the layout
 * of PolynomialOne.coefs[0,:] (src/d2d/trajectory.py:47-72), K samples on
 * linspace(t0,t1,K) (planner_timing, src/d2d/opty_utils.py:8-14), flat outputs -> (va,phi)
 * through DiffFlatness.state_and_input_from_output (src/d2d/guidance.py:22-47), residual
 * rows from CostInput (src/d2d/opty_utils.py:85-97) and CostObstacle kind 1 (:99-134),
 * waypoints from triangle() (:171-187).  The C^3 junction conditions and the end
 * conditions (x,y,psi)(t0),(t1) (src/single_opt_planner.py:46-49, speed = vref) are
 * eliminated: z_axis = Zp d_axis + Z q_axis with nq = 4*S reduced unknowns per axis.
 * ------------------------------------------------------------------------------------ */

/* one scenario row: double[D2D_SCEN_STRIDE] per trajectory (dev [B][D2D_SCEN_STRIDE]) */
#define D2D_SCEN_STRIDE 80
#define D2D_MAX_OBS 16         /* static obstacles per trajectory (CostObstacles, src/d2d/opty_utils.py:136-147;
                                 the reference's largest scenario list, exp_5, holds 12)                   */
enum {
  D2D_SC_X0 = 0, D2D_SC_Y0, D2D_SC_PSI0, D2D_SC_X1, D2D_SC_Y1, D2D_SC_PSI1,
  D2D_SC_VREF,  /* end-condition speed and 'tri' waypoint speed                */
  D2D_SC_VSP,   /* CostInput.vsp                                               */
  D2D_SC_KV, D2D_SC_KPHI, D2D_SC_KOBS,
  D2D_SC_S,     /* obj_scale / K                                               */
  D2D_SC_WWP,   /* waypoint row weight                                         */
  D2D_SC_WX, D2D_SC_WY,   /* wind                                              */
  D2D_SC_GOLEFT,          /* triangle(go_left)                                 */
  D2D_SC_O0X, D2D_SC_O0Y, D2D_SC_O0R,   /* obstacle 0 (r<=0: absent)           */
  D2D_SC_O1X, D2D_SC_O1Y, D2D_SC_O1R,   /* obstacle 1                          */
  D2D_SC_WBND,  /* weight of the soft bound rows                                 */
  D2D_SC_PHIMAX, D2D_SC_VMIN, D2D_SC_VMAX,   /* bounds of those rows: |phi| <= PHIMAX,
                   VMIN <= va <= VMAX (phi_constraint / v_constraint of the scenario)   */
  D2D_SC_KCOL, D2D_SC_RCOL,  /* collision rows between the aircraft of one group: weight, radius */
  D2D_SC_SCOL,  /* their scale, obj_scale / K (src/d2d/multiopty_utils.py:132: no 1/n_ac)  */
  D2D_SC_PMASK, /* bit j set: coupled with aircraft j of the same group (stored as a double) */
  D2D_SC_OKIND, /* bit i set: obstacle i is CostObstacle kind 0, e = clip(exp(r^2 - d^2), 0, 1e3)
                   (src/d2d/opty_utils.py:108-111); clear: kind 1 (stored as a double)          */
  D2D_SC_BANKMAX, /* != 0: CostBank(use_mean=False): obj_scale*max(phi^2) instead of the mean (:72-73) */
  D2D_SC_OEXT,    /* obstacles 2 .. D2D_MAX_OBS-1: (x, y, r) of obstacle i at D2D_SC_OEXT + 3*(i-2) (r<=0: absent;
                     D2D_SC_OKIND bit i)                                                                        */
  D2D_SC_XMIN = D2D_SC_OEXT + 3 * (D2D_MAX_OBS - 2),
  D2D_SC_XMAX, D2D_SC_YMIN, D2D_SC_YMAX
                  /* x_constraint / y_constraint boxes of the scenario (src/single_opt_planner.py:56-57, src/multi_opt_planner.py:63-64): soft bound
                     rows w_b*dist(x, [XMIN, XMAX]), w_b*dist(y, [YMIN, YMAX]) with the weight D2D_SC_WBND of the
                     phi / v rows; an axis with MIN >= MAX (e.g. both zero) has no box.  The last two columns of
                     the row are reserved (zero).                                                                */
};
#define D2D_FIT_NROW 8        /* residual rows per sample */
#define D2D_FIT_MAX_S 6
#define D2D_FIT_NQ_MAX 24     /* 4*S */

/* Levenberg-Marquardt constants (oracle/fit.py LM_*) */
#define D2D_LM_LAMBDA0 1e-3
#define D2D_LM_LAMBDA_MIN 1e-12
#define D2D_LM_LAMBDA_MAX 1e12
#define D2D_LM_DIAG_FLOOR 1e-30
#define D2D_LM_SO_LAMBDA 1e-4     /* default of d2d_fit_opts.so_lambda */
/* A step whose gain ratio is not positive is shortened along its direction before the damping grows: fraction = minimiser of
 * the parabola through the cost at 0 (value, slope) and at 1, clipped to [BT_MIN, BT_MAX]; then BT_SHRINK of it, not below
 * BT_FLOOR.  A failed factorisation (indefinite exact Hessian) multiplies the damping by FAIL_MULT. */
#define D2D_LM_BT_MIN 0.1
#define D2D_LM_BT_MAX 0.5
#define D2D_LM_BT_SHRINK 0.25
#define D2D_LM_BT_FLOOR 0.02
#define D2D_LM_FAIL_MULT 8.0
/* block Gauss-Seidel over coupled aircraft: a scenario still sweeping after GS_PRIO_AT sweeps raises its wave's priority */
#define D2D_GS_PRIO_AT 40
/* ... and its slow sweeps are followed by a line search on the JOINT cost (own rows of every aircraft + every coupled pair once) along
 * the sweep's direction: from sweep GS_LS_SWEEP0 on, after a sweep that moved >= GS_LS_RATIO x the move of the sweep before it; first
 * length rho / (1 - rho) clipped to [1, GS_LS_FIRST_MAX] (GS_LS_FIRST_MAX when the moves grow), doubled while the joint cost falls (up
 * to GS_LS_MAX), one try at a quarter when the first does not lower it (oracle/fit.py bgs_solve; persistent kernel only) */
#define D2D_GS_LS_SWEEP0 8
#define D2D_GS_LS_RATIO 0.8
#define D2D_GS_LS_FIRST_MAX 8.0
#define D2D_GS_LS_MAX 64.0
enum { D2D_ST_RUNNING = 0, D2D_ST_CONVERGED = 1, D2D_ST_MAXITER = 2, D2D_ST_NONFINITE = 3, D2D_ST_STALLED = 4 };

/* Solver of d2d_fit_solve / d2d_fit_iterate (persistent LM kernel; oracle/fit.py states both on the CPU):
 *  D2D_LM_MODE_MINPACK (default)  MINPACK's lmder restated on the normal equations -- the path the CPU arbiter
 *      scipy.optimize.least_squares(method='lm') follows (unit scaling, factor 100; trust region on the Gauss-Newton model,
 *      lmpar's Newton iteration on the damping, lmder's ratio test and radius update), every decision taken from the Cholesky
 *      factor of J^T J + par I instead of the QR factors of J.  Once the trust region has been inactive for mp_finish accepted
 *      steps in a row (par = 0 and ratio >= 0.75: the basin is decided and Gauss-Newton crawls at its linear rate) the fit is
 *      handed to the second-order loop below, started at lambda0, for the quadratic finish; mp_finish = 0 never hands over
 *      (pure lmder, stopping on mp_ftol / mp_xtol / mp_gtol exactly as MINPACK does).  The same hand-over happens when lmder has
 *      STAGNATED: mp_slow trials in a row, accepted or not, each changed the cost by no more than D2D_LM_MP_SLOW_TOL of itself
 *      without meeting lmder's own stopping tests -- the zig-zag of Gauss-Newton on a large-residual fit (the full step
 *      overshoots, the radius shrinks, a damped step gains 1e-7 ...), which scipy follows for hundreds of evaluations (736 on one
 *      121-node bench scenario) and which is never "calm"; the exact Hessian ends it in a handful of iterations at the same minimum.
 *  D2D_LM_MODE_FAST  Nielsen's gain-ratio damping on (H + lam diag|H|) with shortened steps along a rejected direction and
 *      the second-order term once lam <= so_lambda (rounds 1-2): fewer factorisations per fit, but it reaches another local
 *      minimum than scipy on ~13 % of the synthetic bench scenarios. */
enum { D2D_LM_MODE_MINPACK = 0, D2D_LM_MODE_FAST = 1 };
#define D2D_LM_MP_FINISH 3       /* default of d2d_fit_opts.mp_finish */
#define D2D_LM_MP_SLOW 8         /* default of d2d_fit_opts.mp_slow */
#define D2D_LM_MP_SLOW_TOL 1e-4  /* a trial is "slow" when it changes the cost by no more than this fraction (|actred| of lmder) */
#define D2D_LM_SLICE 0           /* default of d2d_fit_opts.slice */
typedef struct {
  int32_t max_iter;     /* trial points (damped solves in FAST mode) per trajectory (default 200)      */
  int32_t check_every;  /* host convergence poll period in iterations (default 8)      */
  double ftol, gtol, xtol;   /* second-order / FAST loop: defaults 1e-14, 1e-9, 1e-11                  */
  double so_lambda;     /* FAST mode: once the damping has fallen to this value the next evaluation carries the
                           second-order term sum_i r_i Hessian(r_i) (exact Hessian of 0.5 sum r^2) beside
                           J^T J: Gauss-Newton's linear rate on these large-residual fits becomes
                           quadratic.  0 = Gauss-Newton only; default D2D_LM_SO_LAMBDA.  Persistent LM
                           kernels only; the launch-pair path ignores it.  (The finish of MINPACK mode always
                           carries the term.)                                                          */
  int32_t mode;         /* D2D_LM_MODE_*: both persistent kernels (K <= 64 fused, and the long-horizon / S != 6 one) honour it;
                           the launch-pair path and coupled groups run FAST                              */
  int32_t mp_finish;    /* MINPACK mode: calm steps before the second-order finish (default D2D_LM_MP_FINISH; 0 = never) */
  double mp_ftol, mp_xtol, mp_gtol;   /* lmder's ftol / xtol / gtol (default 1e-15 each: what bench.py's scipy leg uses) */
  int32_t slice;        /* scheduling of the persistent kernel, > 0: a fit that has run this many iterations while other fits
                           are waiting for a wavefront goes to the back of a device-wide ring (its state is saved, another
                           wavefront resumes it), so that every fit of a batch advances at the same rate whatever the order
                           they were handed out in.  Results are bit-identical.  Measured: equal shares end
                           a 4096-fit launch at (longest fit) + (the excess of the first rounds) -- 1.5 % sooner than running
                           every fit to its end in index order, 4 % later at 32 768 fits -- so the default is 0 = off     */
  int32_t mp_slow;      /* MINPACK mode: stagnating trials in a row before the second-order finish (default D2D_LM_MP_SLOW; 0 = never;
                           only with mp_finish > 0).  (Was `reserved`, always 0, up to version 106.)                          */
  /* ---- version 108: what used to be process-wide environment switches (D2D_LM_PRIO_AT, D2D_GROUPS_LS*, D2D_GROUPS_PRIO_AT,
   * D2D_GROUPS_PAIRS) is part of the call; d2d_fit_opts_default() fills every field with the defaults named here ---- */
  int32_t handout;      /* order in which the persistent kernels hand the fits of a batch to their wavefronts when the batch is larger
                           than the resident wavefronts (results never depend on it: the fits are independent):
                           D2D_HANDOUT_PREDICTED (default) longest-first by a PREDICTED trial count -- a key computed on the device from
                           each scenario row alone, inside the solve (d2d_fit_plan_set_handout_prior; nothing is known from earlier
                           solves); D2D_HANDOUT_INDEX index order.  An explicit d2d_fit_plan_set_order hint overrides both.        */
  int32_t prio_at;      /* a fit that has used this many trial points raises its wave's priority (s_setprio): the stragglers get the
                           SIMD's issue slots ahead of their co-resident wave (default D2D_LM_PRIO_AT; large = never)               */
  int32_t gs_ls;        /* d2d_fit_solve_groups: 1 (default) line search on the joint cost along slow sweeps, 0 plain block Gauss-Seidel */
  int32_t gs_ls_s0;     /* ... from this sweep on (default D2D_GS_LS_SWEEP0; values < 2 are raised to 2)                             */
  double gs_ls_r0;      /* ... after a sweep that moved >= this fraction of the move of the sweep before (default D2D_GS_LS_RATIO)   */
  int32_t gs_prio_at;   /* a scenario still sweeping after this many sweeps raises its wave's priority (default D2D_GS_PRIO_AT)      */
  int32_t gs_pairs;     /* d2d_fit_solve_groups on plans of the long-horizon kernel: 1 = every visit as launch pairs of the split
                           kernels (where their LDS image holds K) instead of ONE launch of the long kernel (default 0)              */
} d2d_fit_opts;
enum { D2D_HANDOUT_INDEX = 0, D2D_HANDOUT_PREDICTED = 1 };
#define D2D_LM_PRIO_AT 48        /* default of d2d_fit_opts.prio_at */
/* *o = the library's defaults (what a NULL opts pointer means).  Fill it first, then change fields: a struct built by hand from an
 * older header would leave the fields of later versions zero. */
int d2d_fit_opts_default(d2d_fit_opts *o);

/* Build the shared basis block on the host (fp64) and upload it.  wref[3] = weights of the
 * whitening metric sum_d wref[d] Phi_d^T Phi_d.  Synchronous. */
int d2d_fit_plan_create(d2d_ctx *ctx, int S, int K, double duration, const double *wref,
                        d2d_fit_plan **out);
/* The same with the kernel family chosen by the caller (version 108; before: D2D_FIT_KNOT / D2D_FIT_LONG / D2D_FIT_SPLIT /
 * D2D_FIT_LONG_SEG / D2D_FIT_LONG_TABLES in the environment of the process).  popts = NULL: the defaults. */
#define D2D_FIT_KERNEL_AUTO (-1)
typedef struct {
  int32_t kernel;        /* D2D_FIT_KERNEL_AUTO (default): knot for S = 6, K <= 64, long otherwise.  D2D_FIT_KERNEL_FUSED: the q-coordinate
                            fused kernel for the default solver too (S = 6, K <= 64 only); D2D_FIT_KERNEL_LONG: the long-horizon kernel
                            whatever K; D2D_FIT_KERNEL_SPLIT: the launch-pair path (K must fit its LDS image); D2D_FIT_KERNEL_KNOT: as AUTO
                            but D2D_EINVAL when the shape has no knot kernel.  A request the shape cannot serve is D2D_EINVAL.          */
  int32_t long_tables;   /* long-horizon kernel: -1 (default) the segment formulation of csrc/fit_seg.h; 0 / 1 / 2: the table kernels with
                            both tables in global memory / the fp64 block in the LDS / both in the LDS; 3: the table kernels, placement
                            chosen from the LDS footprint (development A/B: tools/bench_long.py, tools/dev_seg.py)                      */
  int32_t reserved[2];   /* zero */
} d2d_fit_plan_opts;
int d2d_fit_plan_create_ex(d2d_ctx *ctx, int S, int K, double duration, const double *wref, const d2d_fit_plan_opts *popts,
                           d2d_fit_plan **out);
int d2d_fit_plan_destroy(d2d_fit_plan *plan);
/* Which kernel d2d_fit_solve runs for this plan (uncoupled): the fused persistent LM kernel (S = 6, K <= 64, everything in
 * LDS), the long-horizon persistent kernel (K > 64: the segment formulation of csrc/fit_seg.h -- Legendre coefficients per segment
 * instead of basis tables, LDS footprint independent of K: any K, e.g. the reference's 101 .. 151-node scenarios and its 50 Hz
 * horizons of 351 .. 1501 nodes; since round 3 also every plan with S != 6: the kernel deals its lanes to any number of segments), or
 * the launch-pair path (d2d_fit_plan_opts.kernel = D2D_FIT_KERNEL_SPLIT).  d2d_fit_eval uses the launch-pair evaluation kernel
 * while the basis block fits the LDS (K <~ 229 at S = 6) and the segment formulation beyond; coupled groups run on the group
 * kernels up to that K and on the long-horizon kernel beyond; d2d_fit_rows / d2d_fit_jtj (the contraction-only pair of the
 * bench) keep the LDS limit (D2D_EINVAL beyond).
 * D2D_FIT_KERNEL_KNOT (round 5): the fused shape (S = 6, K <= 64) with the DEFAULT solver runs in knot coordinates -- the reference's
 * local parameterisation CompositeTraj([MinSnapPoly...]) (src/d2d/trajectory.py:166-208), J^T J block tridiagonal, one MFMA per sample
 * (csrc/fit_knot.hip, oracle/fit_knot.py); D2D_LM_MODE_FAST and the time-sliced hand-out of such a plan stay on the fused q kernel.
 * d2d_fit_plan_opts.kernel = D2D_FIT_KERNEL_FUSED at plan creation keeps the q kernel for the default solver too. */
enum { D2D_FIT_KERNEL_SPLIT = 0, D2D_FIT_KERNEL_FUSED = 1, D2D_FIT_KERNEL_LONG = 2, D2D_FIT_KERNEL_KNOT = 3 };
int d2d_fit_plan_kernel(const d2d_fit_plan *plan);
/* The sample geometry of a knot-coordinate plan (version 119; a host function: no context, no GPU).  k0 [S+1]: the first sample of
 * every segment, k0[S] = K; seg_min / seg_max: samples of its shortest / longest segment; seg_floor: the compile-time floor on the
 * shortest segment that the plan's launches of fit_lm_knot_kernel are instantiated with (csrc/fit_knot.hip: the evaluation's
 * J^T r and J^T J run as one straight-line pass then), 0 for the generic instantiation.  Any pointer may be NULL. */
int d2d_fit_knot_segments(int S, int K, double duration, int32_t *k0, int32_t *seg_min, int32_t *seg_max, int32_t *seg_floor);

/* Copy the basis to host buffers (any may be NULL): G [3][K][nq], Gp [3][K][4],
 * Z [8S][nq], Zp [8S][4], Pinit [nq][K]. */
int d2d_fit_plan_get(const d2d_fit_plan *plan, double *G, double *Gp, double *Z, double *Zp,
                     double *Pinit);

/* q0 = projection of the 'tri' waypoints on the basis.  scen dev [B][32]; q dev [B][2*nq]. */
int d2d_fit_init(d2d_ctx *ctx, const d2d_fit_plan *plan, int B, const double *scen, double *q);

/* q0 = least-squares projection of caller-supplied node positions xy dev [B][2][K] (the x and
 * y blocks of an initial-guess vector as Planner.get_initial_guess builds it,
 * src/single_opt_planner.py:79-115) on the basis. */
int d2d_fit_project(d2d_ctx *ctx, const d2d_fit_plan *plan, int B, const double *scen, const double *xy,
                    double *q);

/* One evaluation at q: cost = sum r^2 (fp64), g = J^T r (fp64, dev [B][2nq]), H = J^T J
 * (fp32 via v_mfma_f32_16x16x4_f32, dev [B][2nq][2nq]).  Any output may be NULL. */
int d2d_fit_eval(d2d_ctx *ctx, const d2d_fit_plan *plan, int B, const double *scen,
                 const double *q, double *cost, double *g, float *H);

/* The two halves of d2d_fit_eval as separate launches.  d2d_fit_rows evaluates the residual rows at q -- cost and
 * g = J^T r as d2d_fit_eval (either may be NULL) -- and leaves the fp32 row records (four contracted rows per sample:
 * airspeed, bank and the two position rows) in the plan's scratch, [B][K+1][4] x 16 B in HBM.
 * d2d_fit_jtj contracts the records of the last d2d_fit_rows(B) into J^T J: ONE kernel whose whole duration is the
 * MFMA contraction (records HBM -> LDS, v_mfma_f32_16x16x4_f32, tiles -> HBM) -- the kernel bench.py prices against
 * the fp32 MFMA peak.  H dev [B][2nq][2nq] or NULL (NULL: the tiles stay in the plan's scratch).  Same cost
 * plug-ins as d2d_fit_eval (CostInput, CostObstacle: src/d2d/opty_utils.py:85-134); uncoupled plans only. */
int d2d_fit_rows(d2d_ctx *ctx, d2d_fit_plan *plan, int B, const double *scen, const double *q, double *cost, double *g);
int d2d_fit_jtj(d2d_ctx *ctx, d2d_fit_plan *plan, int B, float *H);

/* Full Levenberg-Marquardt solve from q (in/out).  cost dev [B], iters / status dev int32 [B]
 * (any may be NULL).  stats host double[4] (may be NULL): sum cost, max |J^T r|_inf,
 * trajectories that ended neither D2D_ST_CONVERGED nor D2D_ST_STALLED, evaluations performed (in units of one Gauss-Newton
 * evaluation = 200 contracted rows at K = 50; an evaluation with the second-order blocks contracts 1.5 times as many and counts
 * 1.5) -- the local contribution to the cross-GPU convergence all-reduce.  Synchronises the stream before returning.
 *
 * Terminal states of a fit (every kernel of the family -- knot, fused, long horizon, launch pairs -- keeps them; the reference is
 * oracle/fit.py lm_solve / solve_minpack and oracle/fit_knot.py solve_minpack_knot; tests/test_fit_terminal_cpu.py,
 * tests/test_gpu_fit_terminal.py):
 *   D2D_ST_CONVERGED, D2D_ST_STALLED   the solver's own stop tests; q is the last accepted point, cost the cost there.
 *   D2D_ST_NONFINITE   a REFUSED fit: its first evaluation is not finite -- a NaN or inf anywhere its row is read (end poses, wind,
 *                      weights), or a finite row whose cost overflows.  iters = 0; cost is the non-finite value of that evaluation
 *                      (NaN for a NaN input; +inf for an overflow; an inf input gives NaN or inf as the arithmetic has it); its q row
 *                      keeps the caller's bits; its J^T r is unspecified.  It is never RUNNING: the
 *                      count of d2d_fit_iterate leaves it out, every loop on that count ends.  The other fits of the launch
 *                      have the bits they have when the bad rows are replaced by healthy ones, whatever the hand-out order.
 *   D2D_ST_MAXITER     a CAPPED fit: it has used exactly opts->max_iter trial points (iters == max_iter) and none of the stop
 *                      tests held.  q is the last accepted point (the start point if no trial was accepted), cost the cost there:
 *                      never above the cost at the start.  Every other status comes with iters <= max_iter.
 * stats: [0] sums the FINITE costs only (a refused fit adds nothing: one refusal does not turn the batch's sum, or the job's
 * all-reduced sum, into NaN; without refusals nothing differs), [1] is the largest finite |J^T r| entry of the fits that were not
 * refused, [2] counts the fits
 * that ended neither CONVERGED nor STALLED -- capped and refused fits (and, from d2d_fit_finish before the cap, the running ones):
 * a count of unsettled fits, not a loop condition.  Loop on d2d_fit_iterate's n_running. */
int d2d_fit_solve(d2d_ctx *ctx, const d2d_fit_plan *plan, int B, const double *scen, double *q,
                  const d2d_fit_opts *opts, double *cost, int32_t *iters, int32_t *status,
                  double *stats);

/* The same loop in three parts, for callers that interleave their own convergence check
 * (the cross-GPU all-reduce of the statistics): begin resets the per-trajectory LM state;
 * iterate runs up to n_iters more damped solves (never beyond opts->max_iter in total) and,
 * if n_running != NULL, synchronises and returns how many trajectories are still running (once max_iter is
 * reached it returns 0 without synchronising); finish refreshes cost / J^T r and exports as d2d_fit_solve.
 * n_running counts D2D_ST_RUNNING alone: a refused fit (D2D_ST_NONFINITE, see d2d_fit_solve) leaves the count at its first
 * evaluation, a capped one at max_iter, so `while (n_running > 0)` ends whatever the rows hold.  d2d_fit_finish before the cap
 * exports the fits that were still running as they stand -- D2D_ST_RUNNING, iters = the trials used, q the last accepted point,
 * cost the cost there: bit for bit the q and cost of a solve capped at that many trials by max_iter, which names the same fits
 * D2D_ST_MAXITER -- and counts them in stats[2].
 * Between begin and finish the solve owns q: every d2d_fit_iterate and the d2d_fit_finish of one solve take the SAME q buffer
 * (another pointer is D2D_EINVAL -- the persistent kernels keep the state of the fits that are still running against it, the knot
 * kernel in its own coordinates, so an edited or swapped buffer would be ignored) and options that select the same kernel (a change
 * of mode or slice that would move the solve to another kernel mid-way is D2D_ESTATE). */
int d2d_fit_begin(d2d_ctx *ctx, d2d_fit_plan *plan, int B);
int d2d_fit_iterate(d2d_ctx *ctx, d2d_fit_plan *plan, int B, const double *scen, double *q,
                    const d2d_fit_opts *opts, int n_iters, int32_t *n_running);
int d2d_fit_finish(d2d_ctx *ctx, d2d_fit_plan *plan, int B, const double *scen, const double *q,
                   double *cost, int32_t *iters, int32_t *status, double *stats);

/* Scheduling hint for d2d_fit_solve / d2d_fit_iterate on batches of B trajectories: iters dev int32 [B] = the iteration
 * counts a previous solve of the same scenarios returned (receding-horizon replanning, repeated solves of one batch).  The
 * persistent LM kernel then hands the fits out longest-first, so the launch does not end on one long fit that was drawn late.
 * Results do not depend on it (the fits are independent).  iters = NULL clears the hint; a batch of another size ignores it. */
int d2d_fit_plan_set_order(d2d_ctx *ctx, d2d_fit_plan *plan, int B, const int32_t *iters);
/* The hand-out prior behind D2D_HANDOUT_PREDICTED: how many trial points a fit is EXPECTED to need, as a function of the scenario
 * row alone.  What decides it on the SURVEY 8d workload is how far the two end headings are from the legs of the 'tri' dog-leg the
 * fit starts from (src/d2d/opty_utils.py:171-187) -- near two critical misalignments the start point sits on the watershed between
 * turning left and turning right, lmder stagnates there and the finish walks down a saddle -- and the chord length; the obstacles
 * barely matter (tools/fit_handout_prior.py: rank correlation with the measured trial counts 0.6 on held-out scenarios).  Key of a fit:
 *   table[0][bin(t0)][bin(x)] + table[1][bin(t1)][bin(x)],   x = |p1 - p0| / (vref * duration),
 *   t0 = wrap(psi0 - (beta + a)), t1 = wrap(psi1 - (beta - a)),  beta = heading of the chord, a = go_left * atan(2 h / |p1 - p0|) the
 *   angle of the dog-leg's legs against the chord (h = its apex height, sqrt(max(D^2 - d^2, 0)) / 2),
 * angles in D2D_HANDOUT_NB bins over [-pi, pi), x in D2D_HANDOUT_ND bins over [D2D_HANDOUT_X_LO, D2D_HANDOUT_X_HI) (clamped).  The device
 * computes the keys and a counting sort of them at the start of every solve whose batch exceeds the resident wavefronts (two small
 * launches on the solve's stream, inside whatever the caller times).  table: HOST float [2][D2D_HANDOUT_NB][D2D_HANDOUT_ND], in trial
 * points relative to any common offset; NULL restores the built-in table (csrc/fit_handout_prior.h: regressed on 196 608 synthetic
 * scenarios of OTHER seeds than any bench or test batch).  The built-in table was regressed on the fused shape (S = 6, K <= 64, default
 * solver) and says nothing about other horizons (rank correlation with the trial counts of 121- / 301-node fits: -0.13 / 0.06): plans of
 * the long-horizon kernel hand out in index order until the caller installs a table regressed on solves of their own workload (one
 * solve of a few thousand scenarios is enough: d2dhip/handout.py fit_prior, FitPlan.learn_handout_prior).  A prior only schedules:
 * results are bit-identical whatever it says. */
#define D2D_HANDOUT_NB 48
#define D2D_HANDOUT_ND 12
#define D2D_HANDOUT_X_LO 0.4
#define D2D_HANDOUT_X_HI 1.0
int d2d_fit_plan_set_handout_prior(d2d_ctx *ctx, d2d_fit_plan *plan, const float *table);
/* The hand-out order the LAST solve launch of this plan used over B trajectories: order HOST int32 [B] (position i took trajectory
 * order[i]); D2D_ESTATE if that launch ran in index order or over another batch size.  Synchronous (tests, diagnostics). */
int d2d_fit_plan_get_order(d2d_ctx *ctx, d2d_fit_plan *plan, int B, int32_t *order);
/* The same hint for d2d_fit_solve_groups over R scenarios: from_last != 0 orders the next solves by the sweep counts the
 * LAST d2d_fit_solve_groups of this plan (same R) recorded, longest first; 0 clears it.  Results do not depend on it (the
 * scenarios are independent).  D2D_ESTATE if the plan holds no sweep counts for R scenarios. */
int d2d_fit_plan_set_group_order(d2d_ctx *ctx, d2d_fit_plan *plan, int R, int from_last);

/* Coupled groups (BASELINE configs[2], multi_opt_planner): trajectories g*n_ac .. g*n_ac+n_ac-1 are
 * the aircraft of one scenario and repel each other through CostCollision rows
 * (src/d2d/multiopty_utils.py:120-153; D2D_SC_KCOL/RCOL/SCOL/PMASK select weight, radius, scale and
 * partners).  d2d_fit_plan_set_groups(n_ac <= 8) sizes the kernels' LDS for the extra rows;
 * d2d_fit_solve_groups runs block Gauss-Seidel over the aircraft index (all R groups in one batch
 * per visit, the others' sampled positions frozen, LM state restarted, at most inner_iters damped
 * solves per visit) until no unknown moved by more than tol*(1+|q|) in a sweep or max_sweeps.
 * scen dev [R*n_ac][32], q dev [R*n_ac][2nq] in/out, cost dev [R*n_ac] (per-aircraft sub-problem cost:
 * own rows + its collision rows) or NULL, sweeps_done host or NULL, stats host [4] or NULL
 * (sum of sub-problem costs, max |J^T r|, last sweep's largest relative move, evaluations).
 * Synchronises the stream. */
int d2d_fit_plan_set_groups(d2d_fit_plan *plan, int n_ac);
int d2d_fit_solve_groups(d2d_ctx *ctx, d2d_fit_plan *plan, int R, const double *scen, double *q,
                         const d2d_fit_opts *opts, int max_sweeps, int inner_iters, double tol,
                         double *cost, int32_t *sweeps_done, double *stats);
/* Per-scenario report of the last d2d_fit_solve_groups of this plan (persistent-kernel path): sweeps HOST int32 [R] = sweeps each
 * scenario used, moved HOST double [R] = its largest relative move in the last of them (<= tol: settled); either may be NULL.
 * D2D_ESTATE if the plan holds no such solve over R scenarios.  Synchronous.
 * A REFUSED scenario reports sweeps = 0 and moved = NaN: a scenario is refused whole when the first evaluation of any of its
 * aircraft is not finite (d2d_fit_solve's D2D_ST_NONFINITE; the partners of an aircraft with a NaN end pose read NaN positions).
 * No aircraft of it is visited, every q row of it keeps the caller's bits, its costs are the non-finite values of that
 * evaluation (a finite one for an aircraft that is not coupled to the bad one), and d2d_fit_solve_groups' stats leave it out:
 * [0] sums the finite costs, [2] is the largest move of the scenarios that swept.  The other scenarios of the launch are
 * bit for bit what they are beside a healthy row. */
int d2d_fit_group_report(d2d_ctx *ctx, d2d_fit_plan *plan, int R, int32_t *sweeps, double *moved);

/* Per-launch timing of the LM loop with HIP events on the context's stream: enable = 1
 * starts a fresh recording, 0 stops (d2d_fit_eval's kernel launch is recorded too, as a fit_eval launch).
 * d2d_fit_profile_read waits for the recorded events:
 * out[8]: [0] = sum of fit_eval (J^T J) kernel ms, [1] = its launches, [2] = sum of fit_step kernel
 * ms, [3] = its launches, [4] = sum of fit_lm (fused persistent LM loop) kernel ms, [5] = its launches,
 * [6] = sum of fit_jtj (contraction-only, d2d_fit_jtj) kernel ms, [7] = its launches. */
int d2d_fit_profile(d2d_fit_plan *plan, int enable);
int d2d_fit_profile_read(d2d_fit_plan *plan, double *out);

/* Map q back to monomial coefficients z dev [B][2][S][8] (axis, segment, power). */
int d2d_fit_coeffs(d2d_ctx *ctx, const d2d_fit_plan *plan, int B, const double *scen,
                   const double *q, double *z);

/* Sample a coefficient set: flat outputs and states at the K plan nodes.
 * Y dev [B][6][K] (x,y,xd,yd,xdd,ydd) and Xs dev [B][5][K] (x,y,psi,phi,v); may be NULL. */
int d2d_fit_sample(d2d_ctx *ctx, const d2d_fit_plan *plan, int B, const double *scen,
                   const double *q, double *Y, double *Xs);

/* ------------------------------------------------------------------------------------
 * Direct-collocation NLP in the reference's own parameterisation: the solve behind
 * `opty.direct_collocation.Problem(obj, obj_grad, eom, state_symbols, num_nodes, time_step, known_parameter_map,
 * instance_constraints, bounds)` + `.solve(x0)` (src/single_opt_planner.py:62-71,124; src/multi_opt_planner.py:69-78,86).
 *   unknowns     node values (x, y, psi, phi, v)(t_i), i = 0..N-1 (the reference's free vector, src/single_opt_planner.py:35-39)
 *   equalities   backward-Euler collocation of the symbolic model (src/d2d/opty_utils.py:38-50, +wind sign quirk), i = 1..N-1:
 *                (x_i - x_{i-1})/h - v_i cos psi_i + wx = 0, (y_i - y_{i-1})/h - v_i sin psi_i + wy = 0,
 *                (psi_i - psi_{i-1})/h - g/v_i tan phi_i = 0;  end conditions (x, y, psi)(t0) = p0, (t1) = p1 (:46-49)
 *   bounds       HARD boxes on phi, v and optionally x, y (:53-57)
 *   objective    the cost plug-ins (CostInput / CostAirVel / CostBank mean / CostObstacle(s) / CostComposit,
 *                src/d2d/opty_utils.py:55-165; one CostCollision partner, src/d2d/multiopty_utils.py:120-153) with the gradient
 *                the reference hands to IPOPT (cost_grad, incl. the missing (k/r)^2 of CostObstacle kind 1: the solver therefore
 *                minimises the objective whose gradient that is; the cost REPORTED is the reference's cost()).
 * Solver (oracle/nlp.py is its CPU statement): equalities by an augmented Lagrangian, bounds by a primal-dual log barrier,
 * damped Newton steps on the block-tridiagonal (5x5 blocks) Lagrangian Hessian.  One problem per wavefront: merit function,
 * assembly, the elimination of (phi, v), ratio tests and updates run with lane = node; the 3x3 block recursion that remains is
 * serial in the nodes and runs from both ends of the horizon towards the middle in the two halves of the wave.
 * scen dev [B][D2D_SCEN_STRIDE]: the fit's scenario rows (end poses, VSP, KV, KPHI, KOBS, S, wind, obstacles + OKIND, PHIMAX,
 * VMIN/VMAX, the x/y box, KCOL/RCOL/SCOL); W dev [B][5][N] node values (problem, component, node), in: the initial guess (e.g.
 * Planner.get_initial_guess), out: the solution; partner dev [B][2][N] frozen positions of the CostCollision partner or NULL;
 * work dev double[d2d_nlp_workspace_doubles(N) * B] (scratch: the launch is persistent and uses one workspace per resident wavefront, the
 * first min(B, wave slots) of them; nothing in it is an output); mult dev [B][3][N] or NULL: out, scaled multiplier estimates (node 0 unused;
 * Lagrange multiplier = 2 rho mu);  cost dev [B] (the reference's cost() at the solution), feas dev [B] (largest collocation
 * residual, in the reference's form), iters / status dev int32 [B] or NULL (Newton steps; D2D_ST_CONVERGED / D2D_ST_MAXITER /
 * D2D_ST_STALLED: no feasible point found -- the violation stopped shrinking at the largest penalty).
 * Asynchronous on the context's stream. */
#define D2D_NLP_RHO0 10.0
#define D2D_NLP_RHO_MAX 1e8
#define D2D_NLP_RHO_GROW 10.0
#define D2D_NLP_MUB0 0.1
#define D2D_NLP_MUB_MIN 1e-9
#define D2D_NLP_GRAD_FLOOR 1e-11   /* x rho: rounding floor of the penalty gradient */
#define D2D_NLP_GATE_PROGRESS 1e-9  /* relative decrease of the merit function over inner_max steps below which an unsolved inner problem is left */
#define D2D_NLP_BANKMAX_VALUE_TOL 1e-7   /* CostBank max mode (D2D_SC_BANKMAX rows): converged in value -- feasible, barrier at its floor, a batch of
                                           inner_max steps lowered the merit function by no more than this fraction (the one-hot cost_grad has no zero) */
#define D2D_NLP_BANKMAX_BATCHES 3    /* ... over a window of this many batches of inner_max steps (a D2D_SC_BANKMAX row runs them as one batch) */
#define D2D_NLP_STALL_OUTERS 5      /* solved inner problems in a row that did not halve the violation: D2D_ST_STALLED */
/* Newton steps between two looks at the schedule (multipliers, penalty, barrier parameter) and the number of such looks.  A batch
 * of steps that leaves its inner problem unsolved is followed by another one under the same parameters only while it still lowers
 * the merit function (D2D_NLP_GATE_PROGRESS): with batches of 20 the rare problems whose inner iteration crawls are moved on 3 x
 * sooner than with the 60 of rounds 2-3 (4096 perturbed exp_14: longest problem 481 -> 260 steps, mean 152 unchanged, the same
 * problems converge to the same costs within 5e-10, the reference's 32 catalogue cases keep status and cost) -- and the
 * longest problem is what a batch launch waits for. */
#define D2D_NLP_INNER_MAX 20
#define D2D_NLP_OUTER_MAX 120
typedef struct {
  double rho0;       /* initial penalty (D2D_NLP_RHO0)                                                        */
  double mub0;       /* initial barrier parameter (D2D_NLP_MUB0)                                              */
  double mub_min;    /* final barrier parameter (D2D_NLP_MUB_MIN)                                             */
  double feas_tol;   /* largest collocation residual at convergence (default 1e-9; IPOPT's runs: tol 1e-5)    */
  double opt_tol;    /* barrier KKT error of the last inner problem (default 1e-7)                            */
  int32_t inner_max; /* Newton steps per outer iteration (D2D_NLP_INNER_MAX)                                    */
  int32_t outer_max; /* outer iterations: multiplier / barrier updates (D2D_NLP_OUTER_MAX)                     */
  int32_t serial;    /* solver of the reduced block-tridiagonal system of a Newton step: 0 (default) block cyclic reduction -- log2 N
                        levels of independent 3x3 eliminations, one lane per node; 1 the twisted serial block recursion of round 2
                        (N/2 dependent block pivots).  Same step to rounding.                                   */
  int32_t slots;     /* resident wavefronts (= workspaces) of the persistent launch; 0 (default) = every wave slot of the device
                        (version 108; before: D2D_NLP_SLOTS in the environment.  Was `reserved`, always 0.)                 */
  const double *bounds; /* dev [B][4] = (phi_lo, phi_hi, psi_lo, psi_hi) per problem, or NULL.  phi_lo < phi_hi replaces the symmetric
                           |phi| <= D2D_SC_PHIMAX of the scenario row (opty's bounds dict may hold any interval,
                           src/single_opt_planner.py:53); psi_lo < psi_hi adds a box on the heading of the free nodes (none
                           otherwise; the end headings are equalities).                                             */
  const int32_t *order; /* dev [B]: a permutation of 0 .. B-1, the order in which the persistent launch hands the problems to its
                           resident wavefronts (longest first is what shortens a launch that holds a few problems per wavefront:
                           e.g. the argsort of the previous solve's `iters`, descending), or NULL: index order.  Scheduling only:
                           every problem's result is the same whatever the order.  An entry outside 0 .. B-1 is skipped (the
                           problem it should have named is not solved); an index named twice is the caller's error (two
                           wavefronts would write the same W).  4096 perturbed exp_14: 168 k -> 205 k problems/s.  (version 109) */
} d2d_nlp_opts;
int d2d_nlp_workspace_doubles(int N);
/* A problem whose row is unusable -- PHIMAX <= 0, VMIN <= 0 or VMIN >= VMAX (the model divides by v and the barrier needs an
 * interior), an inverted position box, non-finite end poses -- is refused at once: status D2D_ST_NONFINITE, cost = feas = NaN. */
int d2d_nlp_solve(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W,
                  const double *partner, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                  int32_t *status);

/* The reference's multi-aircraft Problem (src/multi_opt_planner.py:41-78,86: one NLP over the n_ac aircraft of a scenario) for R
 * scenarios in ONE launch: problems r*n_ac .. r*n_ac + n_ac - 1 (rows of scen, W, cost, ...) are the aircraft of scenario r.  The
 * aircraft are coupled through the objective only -- CostCollision on the pair (0, 1), src/d2d/multiopty_utils.py:120-153
 * (D2D_SC_KCOL / RCOL / SCOL of rows 0 and 1; KCOL = 0 on the scenario's first row: uncoupled) -- so a fixed point of block
 * Gauss-Seidel over the aircraft, each block the full collocation solve of one aircraft against the partner's frozen node
 * positions, is a KKT point of the joint problem.  A workgroup takes a scenario, wavefront a its aircraft a: every aircraft is solved
 * uncoupled first (concurrently), then aircraft 0 and 1 take turns until neither moved by more than tol (metres) in a sweep or
 * max_sweeps; no host round trips.  A pair that has not settled reports D2D_ST_MAXITER.
 * work dev double[(d2d_nlp_workspace_doubles(N) * n_ac + 2 * N) * R]; sweeps dev int32 [R], moved dev [R] (largest move of the last sweep)
 * or NULL; the other arguments as d2d_nlp_solve with B = R * n_ac.  Asynchronous on the context's stream. */
int d2d_nlp_solve_groups(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                         double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status,
                         int32_t *sweeps, double *moved);

/* The collocation NLP of d2d_nlp_solve under an objective the library cannot evaluate: the solve behind
 * `opty.direct_collocation.Problem(obj, obj_grad, ...)` when obj / obj_grad are a user's cost plug-in (any object with cost(free,
 * planner) and cost_grad(free, planner), src/single_opt_planner.py:62-71; src/test/test_objective.py:11-16) or plain callables.
 * The host evaluates the user's functions; the device solves one subproblem of the host's sequence of quadratic models
 * (opty/direct_collocation.py), with the exact feasible set:
 *   minimise  sum_i g_i.(W_i - Wc_i) + 1/2 (W_i - Wc_i)^T H_i (W_i - Wc_i)   (+ the structured terms of the row: the host zeroes them)
 *   subject to the collocation equalities, the end conditions and the hard boxes of d2d_nlp_solve.
 * model->g  dev [B][5][N]  gradient of the cost at Wc (component planes, as W)
 * model->H  dev [B][15][N] per-node symmetric 5x5 curvature blocks, upper triangle row by row: planes (0,0) (0,1) .. (0,4) (1,1) .. (1,4)
 *                          (2,2) .. (4,4), i.e. plane a*5 - a*(a-1)/2 + (c-a) holds H[a][c], a <= c
 * model->Wc dev [B][5][N]  centre of the model (the host's current iterate)
 * W dev [B][5][N] in: the start (e.g. Wc), out: the solution; cost dev [B]: the model's value at the solution (0 at Wc); scen, opts,
 * work (d2d_nlp_workspace_doubles(N) * B), mult, feas, iters as d2d_nlp_solve (opts->order and opts->slots are not used: one wavefront
 * and one workspace per problem).  status: D2D_ST_CONVERGED / D2D_ST_MAXITER / D2D_ST_STALLED (no feasible point) as d2d_nlp_solve;
 * D2D_ST_NONFINITE (cost = feas = NaN, at once) for an unusable row or a non-finite entry of g, H or Wc.  Asynchronous on the
 * context's stream.  (version 110) */
typedef struct {
  const double *g;
  const double *H;
  const double *Wc;
} d2d_nlp_model;
int d2d_nlp_solve_model(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, const d2d_nlp_model *model,
                        double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status);

/* d2d_nlp_solve in a wind field that varies in space and time: the plug-point `atm.sample_sym(t, x(t), y(t))` inside the reference's
 * equations of motion (src/d2d/opty_utils.py:38-50), as d2d_step_wind is the plug-point sample(t, loc) of its plant.  The equalities read
 *   (x_i - x_{i-1})/h - v_i cos psi_i + wx(t_i, x_i, y_i) = 0,  (y_i - y_{i-1})/h - v_i sin psi_i + wy(t_i, x_i, y_i) = 0,
 * with t_i = t_start + i h (one multiply-add, not accumulated) and + the spline's value (the model's +wind quirk: a plan consistent with
 * a plant that flies F is planned in -F); D2D_SC_WX / D2D_SC_WY of the rows are ignored.  The constraint Jacobian of a node gains
 * d(wx, wy)/d(x, y) on its (x, y) columns and the Lagrangian Hessian the constraint curvature sum_k rho (c + mu)_k Hess(w_k); along a
 * clamped coordinate (outside the spline's box) those derivatives are zero.  The field f is shared by the batch (host struct, cp a device
 * address); an unusable field, or f NULL: D2D_EINVAL, as for the other *_wind entry points.  No partner.  opts (order, slots, bounds,
 * serial, tolerances), W, work, mult, iters, status as d2d_nlp_solve; feas: the largest collocation residual IN THE FIELD; cost: the
 * reference's cost().  tests/nlp_wind_ref.py is the CPU statement.  Asynchronous on the context's stream.  (version 112) */
int d2d_nlp_solve_wind(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W,
                       double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status,
                       const d2d_wind_field *f, double t_start);

/* d2d_nlp_solve with a FREE time step: the solve behind `opty.direct_collocation.Problem(..., node_time_interval=<sympy Symbol>,
 * bounds={h: (lo, hi), ...})` (variable duration: the interval is the last entry of opty's free vector and may carry a bound).  The
 * node count N stays fixed; every problem's interval h is one more unknown, shared by all its equalities
 *   (x_i - x_{i-1})/h - v_i cos psi_i + wx = 0, ... (the rows' constant wind),
 * inside the HARD box h_lo < h < h_hi (same primal-dual log barrier as the node variables, two duals of its own), with the objective
 *   the row's structured cost + k_dur (N - 1) h,   k_dur >= 0  (0: the duration is whatever lets v sit at VSP).
 * The solver's variable is u = 1 / h, in which the equalities are linear (dc/du = the node difference, d2c/du2 = 0, cross curvature
 * +-1).  The Newton system is the block-tridiagonal matrix A of d2d_nlp_solve BORDERED by one column: b = rho J^T dc/du + rho (c + mu)
 * d2c/(du dw) on a node's five variables and its predecessor's (x, y, psi), and the scalar d = rho |dc/du|^2 + k_dur (N - 1) / u^3 + the
 * barrier diagonal of u, damped like A's diagonal (d += lambda max(|d|, 1e-12)).  It is solved by the Schur complement on d,
 *   x0 = A^-1 r / 2,  y = A^-1 b,  du = (r_u / 2 - b.x0) / (d - b.y),  dW = x0 - y du,
 * b passing through the same per-node elimination of (phi, v) as the right-hand side and through a second pass of the block cyclic
 * reduction; d - b.y <= 0 (the bordered matrix is not positive definite) raises the damping like a failed pivot.  The line search
 * reads the equalities at the trial step, the ratio tests and the KKT error include u.  opts->serial = 1 is not available:
 * D2D_EINVAL.  opts->order, slots, bounds and the tolerances as d2d_nlp_solve; no partner, no field, nothing moves, no pins.
 * free_rows dev [B][4] = (h_lo, h_hi, k_dur, h_start); h_start = 0: the start interval is h0, else h_start; either is pushed strictly
 * inside the box.  A problem with h_lo <= 0, h_lo >= h_hi, k_dur < 0, a non-finite entry, or an unusable scenario row is refused on
 * the device at once: D2D_ST_NONFINITE, cost = feas = h_out = NaN, iters = 0, its W untouched; the rest of the launch is solved.
 * h_out dev [B]: the solved interval (strictly inside its box).  cost: the reference's cost() + k_dur (N - 1) h_out; feas: the largest
 * collocation residual at h_out; status D2D_ST_CONVERGED / D2D_ST_MAXITER / D2D_ST_STALLED as d2d_nlp_solve.
 * work dev double[d2d_nlp_free_workspace_doubles(N) * B].  tests/nlp_free_ref.py is the CPU statement.  Asynchronous on the context's
 * stream.  (version 120) */
int d2d_nlp_free_workspace_doubles(int N);
int d2d_nlp_solve_free(d2d_ctx *ctx, int B, int N, double h0, const double *scen, const d2d_nlp_opts *opts,
                       const double *free_rows /* dev [B][4] = (h_lo, h_hi, k_dur, h_start; 0 = h0) */,
                       double *W, double *work, double *mult, double *cost, double *feas,
                       int32_t *iters, int32_t *status, double *h_out /* dev [B] */);

/* d2d_nlp_solve / d2d_nlp_solve_wind OUTSIDE hard keep-out discs.  For problem b, interior node i (x and y free: 1 .. N-2) and disc
 * m = (cx, cy, R) of keep->discs [B][n_keep][3]:   g_im = (x_i - cx)^2 + (y_i - cy)^2 - R^2 > 0,   a true inequality of the NLP, held by
 * the same primal-dual log barrier as the box (a dual z_im > 0 per (node, disc), started at mub / g); a row with R <= 0 is absent.
 * With d = (x_i - cx, y_i - cy) and the step s of (x_i, y_i): the merit gains - mub log g (+inf when a g <= 0), the stationarity rows
 * of (x_i, y_i) - z 2d, the right-hand side + (mub / g) 2d, the KKT error |z g - mub|, and the (x, y) corner of the node's diagonal
 * block the full Hessian (z / g)(2d)(2d)^T - 2 z I -- the second term is the constraint's own, negative, curvature (the feasible set is
 * the OUTSIDE of a disc): a block that it leaves indefinite fails a pivot, the damping is raised eightfold and the system assembled
 * again.  dz = mub / g - z - (z / g) 2 d.s, ratio test and clip to [mub / (1e10 g), 1e10 mub / g] as for the box duals.  The primal
 * fraction-to-the-boundary rule is exact: the smaller positive root a of  g + 2 a d.s + a^2 |s|^2 = (1 - tau) g.
 * Start: after the box push a free node closer than 1.01 R to a centre is moved radially to 1.01 R (along the left normal of the leg
 * p0 -> p1 where |d| < 1e-12 R), discs in index order, two passes, then the box push again.
 * Refused on the device before the problem's first store (D2D_ST_NONFINITE, cost = feas = NaN, iters = 0, W untouched; the rest of the
 * launch is solved): a non-finite entry of a disc, an end pose on or inside a disc, a free node still on or inside a disc after the
 * start rule.  cost is the reference's cost(): the discs add nothing.  The constraint is held AT THE NODES; between two nodes at spacing
 * s the polyline can cut a chord of depth R - sqrt(R^2 - (s/2)^2): the caller inflates R for that (single_opt_planner does).
 * f NULL: the rows' constant wind, and t_start is not read; else t_start dev [B], as d2d_nlp_solve_moving.  f and t_start go together.
 * kwork dev [B][n_keep][N]: the duals z, written by the solve; afterwards the multipliers of the disc constraints (0 at the end nodes and
 * for absent discs).  work dev double[d2d_nlp_workspace_doubles(N) * B].  n_keep = 0: the solve of d2d_nlp_solve / d2d_nlp_solve_wind
 * (kwork may be NULL).  n_keep > D2D_MAX_KEEP or keep NULL: D2D_EINVAL.  opts, W, mult, iters, status as d2d_nlp_solve.
 * tests/nlp_keepout_ref.py is the CPU statement.  Asynchronous on the context's stream.  (version 121) */
#define D2D_MAX_KEEP 8
typedef struct {
  int32_t n_keep, pad;  /* 0 .. D2D_MAX_KEEP */
  const double *discs;  /* dev [B][n_keep][3] = (cx, cy, R) */
} d2d_keep_out;
int d2d_nlp_solve_keepout(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W,
                          double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status,
                          const d2d_wind_field *field, const double *t_start, const d2d_keep_out *keep, double *kwork);

/* d2d_nlp_solve_groups in a wind field: the multi-aircraft Problem of R scenarios whose equalities are those of d2d_nlp_solve_wind,
 *   .. + wx(t_i, x_i, y_i) = 0,  .. + wy(t_i, x_i, y_i) = 0,   t_i = t_start[r] + i h  (one multiply-add, not accumulated),
 * with the field's Jacobian in the constraint Jacobian, its curvature in the Lagrangian Hessian and zero derivatives along a clamped
 * coordinate; D2D_SC_WX / D2D_SC_WY of the rows are not read.  Arguments, workspace size, statuses and the block Gauss-Seidel are
 * d2d_nlp_solve_groups's: sweep 0 uncoupled and concurrent, then aircraft 0 and 1 take turns against the partner's frozen node
 * positions (CostCollision lives in the objective and does not meet the field) until neither moved by more than tol or max_sweeps;
 * an unsettled pair reports D2D_ST_MAXITER.  t_start is a DEVICE array [R], one start time per scenario (full_sim's mission chain
 * computes it from each formation's stop row without a host round trip); a non-finite entry refuses that scenario's aircraft at
 * once (D2D_ST_NONFINITE, cost = feas = NaN, sweeps = 0), like an unusable row.  f NULL, an unusable field or t_start NULL:
 * D2D_EINVAL before anything is launched.  As in d2d_nlp_solve_groups, the last 2 * N doubles per scenario of work (behind the
 * R * n_ac workspaces, scenario r at offset r * 2 * N) are left holding the x and y planes aircraft 1 had before its last turn: the
 * frozen partner that the reported cost of aircraft 0 was evaluated against.  The model ADDS the field: a plan consistent with a plant that flies F is planned in -F.
 * tests/nlp_groups_wind_ref.py is the CPU statement.  Asynchronous on the context's stream.  (version 113) */
int d2d_nlp_solve_groups_wind(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                              double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                              int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start);

/* d2d_nlp_solve_groups / d2d_nlp_solve_groups_wind with collision avoidance on ANY set of aircraft pairs.  D2D_SC_PMASK of aircraft
 * a's row is its partner set (bit j: aircraft j of the same scenario); an aircraft with a non-empty set carries D2D_SC_KCOL / RCOL /
 * SCOL (KCOL = 0: it takes its turns without the term).  Block Gauss-Seidel as before: sweep 0 solves every aircraft uncoupled and
 * concurrently; in sweeps 1.. the aircraft with a non-empty set take turns in index order, each turn a full solve from the
 * aircraft's current nodes against the frozen node positions of ALL its partners (terms summed in ascending partner index); moved is
 * the largest move of any turn of the sweep, and the loop ends at moved <= tol or max_sweeps.  An unsettled scenario reports
 * D2D_ST_MAXITER on the aircraft that took turns.  A fixed point is a KKT point of the joint problem: the coupling is in the
 * objective only.  With the masks 0b10, 0b01 of the pair (0, 1) the results are those of d2d_nlp_solve_groups[_wind] bit for bit.
 * f and t_start both NULL: the rows' constant wind (d2d_nlp_solve_groups); both set: the field, node i of scenario r at
 * t_start[r] + i h (d2d_nlp_solve_groups_wind, same validation); one of them NULL: D2D_EINVAL.
 * Masks are checked on the device, per scenario, before its first solve (no host round trip: the rows may have been finished on
 * the device): an entry that is not an integer in [0, 2^n_ac), a self bit, or a bit j that aircraft j's mask does not return
 * (the term of a pair belongs to both aircraft's objectives or to neither) refuses ALL aircraft of that scenario at once --
 * D2D_ST_NONFINITE, cost = feas = NaN, iters = 0, sweeps = 0, moved = 0, W untouched -- like an unusable row; the other scenarios
 * of the launch are solved.  No mask indexes outside its scenario's W.
 * Arguments and workspace size as d2d_nlp_solve_groups_wind; the last 2 * N doubles per scenario of work hold the x and y planes
 * the aircraft of the last turn had before it.  tests/nlp_groups_pairs_ref.py is the CPU statement.  Asynchronous on the context's
 * stream.  (version 114) */
int d2d_nlp_solve_groups_pairs(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                               double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                               int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start);

/* Moving obstacles of the collocation planner: CostObstacle discs whose centre is piecewise linear in time -- crossing traffic, a
 * formation whose plan is committed, a no-fly disc that drifts.  A moving disc is a static disc of the row (D2D_SC_O0X ..) with the
 * centre c(t_i) of the node's own time t_i = t_start + i h in place of (x, y): the same value, reference cost, gradient and
 * Gauss-Newton block, weighted by the row's D2D_SC_KOBS and D2D_SC_S; its radius and kind are its own.  The tracks live in a side table
 * (the scenario row is full): G = the number of problems (d2d_nlp_solve_moving) or of scenarios (d2d_nlp_solve_groups_moving: all
 * aircraft of a scenario see the same tracks).  Centre at time t: linear between the two knots that bracket t, held at the first or
 * last knot outside them.  Times are absolute, on the clock of t_start and of the wind field.  (version 115) */
#define D2D_MAX_MOV 8            /* moving discs per problem / scenario */
#define D2D_MOV_MAX_KNOT 32
typedef struct {
  int32_t n_mov;        /* 0 .. D2D_MAX_MOV */
  int32_t n_knot;       /* 2 .. D2D_MOV_MAX_KNOT, the same for every track of the call */
  const double *knots;  /* dev [G][n_mov][n_knot][3] = (t, x, y), t strictly increasing */
  const double *disc;   /* dev [G][n_mov][2] = (r, kind); r <= 0: absent; kind 0 / 1: CostObstacle kind 0 / kind 1 (D2D_SC_OKIND) */
} d2d_moving_obstacles;

/* The centres of the moving discs at the node times: ctr dev [G][n_mov][2][N], disc m of problem g at node i = the track at
 * t_start[g] + i h (one multiply-add, not accumulated); t_start dev [G].  This is the pass the two solve entries below run ahead of
 * their solve; it is exported so that it can be tested on its own.  It does not validate the tracks (the solve kernels do).  mov NULL,
 * n_mov or n_knot out of range, or a NULL table, ctr or t_start with n_mov > 0: D2D_EINVAL; n_mov = 0: nothing is written.
 * Asynchronous on the context's stream. */
int d2d_mov_sample(d2d_ctx *ctx, int G, int N, double h, const double *t_start, const d2d_moving_obstacles *mov, double *ctr);

/* d2d_nlp_solve_wind around moving discs.  The arguments of d2d_nlp_solve_wind with three changes: t_start is a DEVICE array [B], one
 * start time per problem; f may be NULL, meaning the rows' constant wind (D2D_SC_WX / D2D_SC_WY); mov are the tracks and mov_work
 * B * n_mov * 2 * N doubles for the centre planes, which d2d_mov_sample's kernel fills on the context's stream ahead of the solve.
 * The objective gains, per node and per disc with r > 0, the static disc's term of that disc's kind, summed in ascending disc index
 * after the row's static discs.  t_start is required whenever n_mov > 0; with n_mov = 0, f and t_start go together (both NULL: the
 * solve of d2d_nlp_solve, bit for bit; both set: that of d2d_nlp_solve_wind).  mov NULL, n_mov or n_knot out of range, or a NULL
 * table or mov_work with n_mov > 0: D2D_EINVAL before anything is launched.
 * The tracks are validated on the device, per problem, before its solve: a non-finite knot, knot times that do not increase strictly,
 * a kind that is neither 0 nor 1 (absent discs included), or a start time that is not finite refuses THAT problem --
 * D2D_ST_NONFINITE, cost = feas = NaN, iters = 0, its W untouched -- and the rest of the launch is solved.
 * tests/nlp_moving_ref.py is the CPU statement.  Asynchronous on the context's stream. */
int d2d_nlp_solve_moving(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W, double *work,
                         double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, const d2d_wind_field *f,
                         const double *t_start, const d2d_moving_obstacles *mov, double *mov_work);

/* d2d_nlp_solve_groups_pairs around moving discs: its arguments (masks in the rows, optional field), plus the tracks of each
 * SCENARIO (G = R) and mov_work of R * n_mov * 2 * N doubles.  Every aircraft of scenario r adds the discs' terms at the node times
 * t_start[r] + i h, in the uncoupled sweep and in every turn; the rules for f, t_start, mov and mov_work are those of
 * d2d_nlp_solve_moving.  An unusable track, or a start time that is not finite, refuses all aircraft of that scenario exactly as a
 * malformed mask does (sweeps = 0, moved = 0, W untouched).  With n_mov = 0, or every r <= 0, the results are those of
 * d2d_nlp_solve_groups_pairs bit for bit.  Asynchronous on the context's stream. */
int d2d_nlp_solve_groups_moving(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                                double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                                int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start,
                                const d2d_moving_obstacles *mov, double *mov_work);

/* d2d_nlp_solve_keepout outside hard discs that MOVE: a committed aircraft is such a disc.  The tracks are a d2d_moving_obstacles table as
 * it is (d2d_fleet_tracks' output goes straight in), read differently: disc[m][0] is the NODE RADIUS R of the hard constraint (R <= 0:
 * the disc is absent), disc[m][1] is validated as in d2d_nlp_solve_moving (0 or 1) and otherwise not read.  For problem b, interior node i
 * and disc m with the centre c_m(t) of d2d_mov_sample:   g_im = |p_i - c_m(t_start[b] + i h)|^2 - R_m^2 > 0.   Merit, stationarity,
 * right-hand side, KKT error, the Newton block, dz, the exact ratio test, the start rule and the dual clip are d2d_nlp_solve_keepout's
 * with the node's own centre in the place of c; the centres are data, no derivative is added.  The row's soft static discs still count;
 * soft moving discs, pins and a free step are not carried.  At most D2D_MAX_MOV (= D2D_MAX_KEEP) discs.
 * Refused per problem before its first store (D2D_ST_NONFINITE, cost = feas = NaN, iters = 0, W untouched, the rest of the launch
 * solved): an unusable track (d2d_nlp_solve_moving's rules), a start time that is not finite, a non-finite R, an end pose with g <= 0
 * at ITS OWN node's time (node 0 at t_start, node N - 1 at t_start + (N - 1) h), a free node with g <= 0 after the start rule.
 * field, t_start: the rules of d2d_nlp_solve_moving (t_start is required when n_mov > 0).  mov_work dev [B][n_mov][2][N]: the centres,
 * written by the sampling pass on the context's stream; kwork dev [B][n_mov][N]: the duals, afterwards the constraints' multipliers.
 * n_mov = 0: the solve of d2d_nlp_solve / d2d_nlp_solve_wind, bit for bit (mov_work and kwork may be NULL).  The constraint holds at the
 * nodes; between two rows the RELATIVE displacement of aircraft and disc cuts the chord: R = sqrt(d^2 + (s / 2)^2) with s the largest
 * relative displacement between two nodes keeps the continuous distance >= d (d2d.opty_utils.MovingKeepOut.lowered).
 * tests/nlp_keepout_moving_ref.py is the CPU statement.  Asynchronous on the context's stream.  (version 126) */
int d2d_nlp_solve_keepout_moving(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W,
                                 double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status,
                                 const d2d_wind_field *field, const double *t_start, const d2d_moving_obstacles *mov, double *mov_work,
                                 double *kwork);

/* d2d_nlp_solve_groups_pairs with every aircraft outside its scenario's hard moving discs: the arguments of d2d_nlp_solve_groups_moving
 * (tracks [R][n_mov][..] per SCENARIO, read as above) plus kwork dev [R n_ac][n_mov][N], every aircraft's own duals.  The block
 * Gauss-Seidel is d2d_nlp_solve_groups_pairs's (masks in the rows, checked on the device); every aircraft of scenario r holds the
 * scenario's discs in the uncoupled sweep and in every turn.  Each turn is a full solve from the aircraft's current nodes: the start rule
 * moves nodes that sit on a boundary back to 1.01 R and the duals restart at mub / g.  A bad track, radius or start time refuses the
 * whole scenario exactly as a malformed mask does, and so does an aircraft whose end pose lies on or inside a disc at its node's time
 * or that the start rule cannot place outside the discs -- decided before the first barrier by every wavefront alike.  That decision
 * is taken on the aircraft's GUESSES.  A later turn starts from the aircraft's current nodes and applies the start rule again; if it
 * cannot place them (a node the partners' term has moved between two overlapping discs, say), that AIRCRAFT alone reports
 * D2D_ST_NONFINITE with NaN cost and feas, its W stays what its previous solve left, the other aircraft go on, and `iters` counts the
 * solves before.  Callers that need all-or-nothing treat any D2D_ST_NONFINITE of a scenario as its refusal (full_sim.deconflict_plans
 * does: the formation keeps its plan and is listed in `refused`).  With n_mov = 0
 * the call is d2d_nlp_solve_groups_pairs; with every R <= 0 its results.  (version 126) */
int d2d_nlp_solve_groups_keepout(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts,
                                 int max_sweeps, double tol, double *W, double *work, double *mult, double *cost, double *feas,
                                 int32_t *iters, int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *field,
                                 const double *t_start, const d2d_moving_obstacles *mov, double *mov_work, double *kwork);

/* d2d_nlp_solve_keepout INSIDE a convex polygon: a geofence.  For problem b, interior node i and edge k = (ax, ay, b, kap) of
 * fence->edges [B][n_edge][4], a the edge's outward unit normal:   g_ik = b_k - (ax_k x_i + ay_k y_i) > 0,   a true inequality of the NLP held
 * by the same primal-dual log barrier as the box and the discs (a dual z_ik > 0 per (node, edge), started at mub / g); a row with
 * ax = ay = 0 is absent.  The constraint is linear, grad g = -a: the merit gains - mub log g (+inf when a g <= 0), the stationarity rows of
 * (x_i, y_i) + z a, the right-hand side - (mub / g) a, the KKT error |z g - mub|, and the (x, y) corner of the node's diagonal block the
 * full Hessian (z / g) a a^T -- positive semidefinite: the edges add no negative curvature.  With the step s of (x_i, y_i):
 * dz = (mub + z a.s) / g - z, ratio test and clip to [mub / (1e10 g), 1e10 mub / g] as for the box duals, and the primal
 * fraction-to-the-boundary rule is a <= tau g / (a.s) where a.s > 0, exact.  Every a.p is taken as fma(ax, x, ay y).
 * Start, behind the discs' rule: two passes over the edges in index order, a free node with g_k < kap_k moves along -a_k to g_k = kap_k;
 * then the box push again.  A guess with g >= kap at every edge (and outside 1.01 R of every disc) is not moved.
 * Refused per problem before its first store (D2D_ST_NONFINITE, cost = feas = NaN, iters = 0, W untouched, the rest of the launch
 * solved): a non-finite entry of an edge, a present edge with | |a| - 1 | > 1e-12 or kap <= 0, an end pose with g <= 0, a free node
 * with g <= 0 at an edge or a disc after the start rules -- and what refuses d2d_nlp_solve_keepout.
 * keep, kwork: the static hard discs of d2d_nlp_solve_keepout, held in the same solve (a permitted area with no-fly zones inside it is
 * one call); keep must not be NULL, n_keep = 0: no discs (discs and kwork may be NULL).  The row's soft static discs still count; moving
 * discs, pins and a free step are not carried.  cost is the reference's cost(): discs and edges add nothing.
 * Guarantee: the feasible set of the edges is convex, so the straight segment between two feasible nodes is feasible -- the whole polyline
 * of a returned plan keeps every g > 0 with no chord inflation (d2d.opty_utils.GeoFence lowers a polygon and a margin to the rows).
 * fwork dev [B][n_edge][N]: the duals z, afterwards the multipliers of the edge constraints (0 at the end nodes and for absent edges).
 * n_edge = 0: the call is d2d_nlp_solve_keepout (edges and fwork may be NULL), and with n_keep = 0 as well d2d_nlp_solve /
 * d2d_nlp_solve_wind.  fence NULL, n_edge outside 0 .. D2D_MAX_FENCE, NULL edges or fwork with n_edge > 0: D2D_EINVAL before any launch.
 * field, t_start, opts, W, work, mult, iters, status as d2d_nlp_solve_keepout.  tests/nlp_fence_ref.py is the CPU statement.
 * Asynchronous on the context's stream.  (version 127) */
#define D2D_MAX_FENCE 8
typedef struct {
  int32_t n_edge, pad;  /* 0 .. D2D_MAX_FENCE */
  const double *edges;  /* dev [B][n_edge][4] = (ax, ay, b, kap) */
} d2d_fence;
int d2d_nlp_solve_fence(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W,
                        double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status,
                        const d2d_wind_field *field, const double *t_start, const d2d_keep_out *keep, double *kwork,
                        const d2d_fence *fence, double *fwork);

/* d2d_nlp_solve_free OUTSIDE static hard keep-out discs and INSIDE a convex geofence: the leg's duration is free while both families of
 * d2d_nlp_solve_fence are held -- the call for a no-fly zone whose detour does not fit a duration guessed in advance.  Formulation: the
 * unknowns, the box of h, the objective (the row's structured cost + k_dur (N - 1) h) and the bordered Newton system of
 * d2d_nlp_solve_free; the inequalities g > 0 of d2d_nlp_solve_keepout (discs) and d2d_nlp_solve_fence (edges) at every interior node,
 * each with its dual on the same primal-dual log barrier.  Discs and edges read (x, y) of the interior nodes alone, so the border
 * column b, the scalar d and the residual of the row of u = 1 / h gain no term: what the families add -- stationarity rows, right-hand
 * side, the (x, y) corner of the node's diagonal block with the discs' - 2 z I, KKT error -- sits in the block-tridiagonal matrix A and is
 * so in BOTH solves of the Schur complement (x0 = A^-1 r / 2 and y = A^-1 b see the same damped matrix).  A failed pivot in either pass
 * of the cyclic reduction (the second factors copies of the same D', E': it can fail only where the first would) or d - b.y <= 0
 * raises the damping eightfold.  The line
 * search reads the equalities at u + a du and the families' barriers at the trial nodes; the step length is the smallest of four ratio
 * tests -- the box, the exact quadratic root of the discs, tau g / (a.s) of the edges, u's -- and every floating-point sum takes the discs
 * in ascending index, then the edges.  Start: box push, the discs' rule, the edges' rule, box push, then the step pushed strictly inside
 * its box; both families' duals start at mub / g.
 * free_rows, h_out, work (d2d_nlp_free_workspace_doubles(N) per problem) and opts as d2d_nlp_solve_free: opts->serial = 1 is D2D_EINVAL,
 * constant wind of the rows, no field, nothing moves, no pins.  keep, kwork, fence, fwork as d2d_nlp_solve_fence (the duals live in
 * kwork dev [B][n_keep][N] and fwork dev [B][n_edge][N], afterwards the multipliers; 0 at the end nodes and for absent rows), with the
 * same D2D_EINVAL cases before any launch: keep or fence NULL, a count outside 0 .. D2D_MAX_KEEP / D2D_MAX_FENCE, a NULL table or dual
 * array with a positive count.  Either count may be 0; with n_keep = 0 AND n_edge = 0 the call is d2d_nlp_solve_free, its kernel and
 * its bytes.  Refused on the device (D2D_ST_NONFINITE, cost = feas = h_out = NaN, iters = 0, W untouched; the rest of the launch is
 * solved): what refuses a problem of d2d_nlp_solve_free, and what refuses one of d2d_nlp_solve_fence.  cost: the reference's cost() +
 * k_dur (N - 1) h_out; discs and edges add nothing.  The discs are held AT THE NODES: a caller that inflates R for the chord between two
 * nodes inflates for the LARGEST step of the box, h_hi (conservative for every h inside); the fence is convex and needs none.
 * tests/nlp_free_fence_ref.py is the CPU statement.  Asynchronous on the context's stream.  (version 129) */
int d2d_nlp_solve_free_fence(d2d_ctx *ctx, int B, int N, double h0, const double *scen, const d2d_nlp_opts *opts,
                             const double *free_rows /* dev [B][4] = (h_lo, h_hi, k_dur, h_start; 0 = h0) */,
                             double *W, double *work, double *mult, double *cost, double *feas,
                             int32_t *iters, int32_t *status, double *h_out /* dev [B] */,
                             const d2d_keep_out *keep, double *kwork, const d2d_fence *fence, double *fwork);

/* d2d_nlp_solve_groups_pairs with every aircraft inside its scenario's convex polygon: the arguments of d2d_nlp_solve_groups_pairs, then
 * fence with edges dev [R][n_edge][4], one polygon per SCENARIO read as above, then fwork dev [R n_ac][n_edge][N], every aircraft's own
 * duals (afterwards the multipliers).  No hard discs are carried.  The block Gauss-Seidel is d2d_nlp_solve_groups_pairs's (masks in the
 * rows, checked on the device); every aircraft holds the scenario's edges in the uncoupled sweep and in every turn.  The constraint is
 * per aircraft, so a fixed point of the alternation is still a KKT point of the joint problem.  Each turn is a full solve from the
 * aircraft's current nodes: the start rule moves nodes closer than kap to an edge back to g = kap and the duals restart at mub / g.
 * A bad edge (the rules above) refuses the whole scenario exactly as a malformed mask does (D2D_ST_NONFINITE, cost = feas = NaN,
 * sweeps = 0, W untouched), and so does an aircraft whose end pose has g <= 0 or whose guess the start rule cannot place inside --
 * decided before the first barrier by every wavefront alike, on the aircraft's GUESSES.  A later turn that cannot start refuses that
 * AIRCRAFT alone, as d2d_nlp_solve_groups_keepout describes.  By convexity every aircraft's polyline stays inside.  n_edge = 0: the
 * call is d2d_nlp_solve_groups_pairs (edges, fwork may be NULL); with every edge absent its bytes.  fence NULL, n_edge outside
 * 0 .. D2D_MAX_FENCE, NULL edges or fwork with n_edge > 0: D2D_EINVAL before any launch.  f NULL: the rows' constant wind (t_start is
 * not read).  tests/nlp_fence_ref.py solve_groups is the CPU statement.  Asynchronous on the context's stream.  (version 127) */
int d2d_nlp_solve_groups_fence(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts,
                               int max_sweeps, double tol, double *W, double *work, double *mult, double *cost, double *feas,
                               int32_t *iters, int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *field,
                               const double *t_start, const d2d_fence *fence, double *fwork);

/* Timed waypoints of the collocation planner: components of x, y, psi of INTERIOR nodes held at given values -- a point to fly
 * through at a given time, a gate, a heading at a hand-over.  A pinned component is a fixed variable exactly as x, y, psi of the two end
 * nodes are: it starts at its value and keeps it (the returned W holds the value bit for bit), has no bound duals and no barrier
 * term, takes no step (an identity row and column in the Newton system, in both factorisations), and is left out of the KKT error and
 * the ratio tests.  The objective's terms -- discs, moving discs, partners -- still count at a pinned node.  The pins live in a side
 * table, one list per problem, padded to a common length with rows of mask 0.  (version 116) */
#define D2D_MAX_VIA 16           /* rows per problem */
typedef struct {
  int32_t n_via;        /* 0 .. D2D_MAX_VIA */
  const double *pts;    /* dev [G][n_via][5] = (node, mask, x, y, psi); mask bit 0 / 1 / 2: x / y / psi is pinned; mask 0: the row is absent */
} d2d_via_points;

/* d2d_nlp_solve_moving through pins: its arguments, with mov NULL allowed (nothing moves), plus the pins of each problem (G = B) and
 * via_work, B * N int32 for the planes of the nodes' fixed sets.  via NULL, n_via out of range, or a NULL table or via_work with
 * n_via > 0: D2D_EINVAL before anything is launched; the other rules are those of d2d_nlp_solve_moving.  With n_via = 0 the call IS
 * d2d_nlp_solve_moving; with every mask 0 its results are bit for bit the same.
 * The pins are validated on the device, per problem, before its solve.  A row with a mask that is no integer in 1 .. 7 (0: absent), a
 * node that is no integer in 1 .. N-2, a pinned value that is not finite or lies outside the problem's box (D2D_SC_XMIN .. YMAX, the
 * psi interval of d2d_nlp_opts.bounds), or a (node, component) that another row pins too refuses THAT problem -- D2D_ST_NONFINITE,
 * cost = feas = NaN, iters = 0, its W untouched -- and the rest of the launch is solved.  The values of components outside a row's
 * mask are not read.  tests/nlp_via_ref.py states the solve on the CPU.  Asynchronous on the context's stream. */
int d2d_nlp_solve_via(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W, double *work,
                      double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, const d2d_wind_field *f,
                      const double *t_start, const d2d_moving_obstacles *mov, double *mov_work, const d2d_via_points *via, int32_t *via_work);

/* d2d_nlp_solve_groups_moving through pins: its arguments, with mov NULL allowed, plus the pins of each AIRCRAFT (G = R * n_ac, the
 * aircraft of a scenario consecutive) and via_work of R * n_ac * N int32.  The rules for via and via_work are those of
 * d2d_nlp_solve_via; an unusable row of any aircraft refuses all aircraft of its scenario exactly as a malformed mask does (sweeps = 0,
 * moved = 0, W untouched).  With n_via = 0 the call IS d2d_nlp_solve_groups_moving; with every mask 0 its results are bit for bit the
 * same.  Asynchronous on the context's stream. */
int d2d_nlp_solve_groups_via(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                             double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                             int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start,
                             const d2d_moving_obstacles *mov, double *mov_work, const d2d_via_points *via, int32_t *via_work);

/* Flight audit: what a flown or planned state history kept of the planners' promises, in one streaming pass over a history that is
 * already on the device.  Per aircraft: the closest approach to the other aircraft of its formation, the clearance from static and
 * from moving discs, the tracking error against the reference it followed, the bank and airspeed envelope.  (version 117)
 * History: X_hist dev [n_rows][5][N], plane-major, planes x, y, psi, phi, v, N = n_form * n_ac, drone d = formation d / n_ac, aircraft
 * d % n_ac -- the layout d2d_sim_gvf_run*, d2d_sim_track_run* and d2d_sim_dfff_run* write (a plan [N][5][K] is transposed by the
 * caller).  Only the planes the requested outputs need are read; psi never is.  Row i of formation f is at t_start[f] + i dt_row
 * (t_start dev [n_form], NULL: 0; dt_row = the step times the history's rec_stride).  rows dev int32 [n_form] (NULL: n_rows) is the
 * number of valid rows of each formation, clamped to 0 .. n_rows: a row at an index >= rows[f] is never read.
 * Between two rows every position is linear in s in [0, 1].  For a relative position p(s) = p0 + s d the closest approach is at
 * s* = clamp(-(p0 . d) / (d . d), 0, 1) (0 when d . d = 0), its distance |p0 + s* d| -- at s* = 0 and s* = 1 the row's own p0 and p1,
 * exactly -- and its time t_start[f] + (i + s*) dt_row.  Minima and maxima are taken over the squared distances and the square root
 * is drawn once, at the end; the counts compare squared distances with d_safe^2, r^2 and err_tol^2.  One valid row: the row is the
 * answer.  No valid row, no partner (n_ac = 1) or an absent disc (r <= 0), "nothing seen": minima +inf, maxima -inf, times NaN,
 * partner -1, counts 0.  Ties: the earliest time wins, among partners at the same time the smallest index.
 * Outputs (d2d_audit_out; any pointer may be NULL: neither computed nor stored), per drone [N] unless noted:
 *   sep_dist, sep_partner, sep_time   the smallest distance over all segments to any other aircraft of the formation, that partner's
 *                                     index in the formation, the time;  sep_count: the valid rows at which the nearest partner is
 *                                     closer than d_safe (d_safe <= 0: no count, 0)
 *   stat_clear, stat_time, stat_count [n_stat][N]: distance to the centre minus r of static disc k, its minimum over the segments, the
 *                                     time, the valid rows with clearance < 0.  stat dev [n_form][n_stat][3] = (x, y, r), r <= 0: absent
 *   mov_clear, mov_time, mov_count    [n_mov][N]: the same for the moving discs of mov (G = n_form).  Their centres at the row times are
 *                                     d2d_mov_sample's (its kernel fills mov_work, n_form * n_mov * 2 * n_rows doubles, on the context's
 *                                     stream ahead of the audit) and a centre is LINEAR BETWEEN ROWS: a track's knot that falls inside a
 *                                     step is cut.  The disc's kind is not used
 *   err_max, err_time, err_count      against x_ref, y_ref dev [n_rows][N] (row i pairs with sample i, as in d2d_sim_track_run): the largest
 *                                     |(x, y) - (x_ref, y_ref)| over the valid ROWS (not between them), its time, the rows above err_tol
 *   phi_max, v_min, v_max             max |phi|, min v, max v over the valid rows
 *   status                            int32 [n_form]: 0, or the D2D_AUDIT_* bits of a refusal
 * Refusals, per formation: a non-finite value in a plane, reference or disc row that the call reads for the valid rows of any of its
 * aircraft (D2D_AUDIT_NONFINITE), a t_start that is not finite (D2D_AUDIT_BAD_TSTART), with n_mov > 0 a track that d2d_nlp_solve_moving
 * would refuse (D2D_AUDIT_BAD_TRACK) -- every floating output of its aircraft NaN, every count and partner -1; the other formations are
 * audited.
 * The rows are cut into blocks of rows_per_block (0: the library's choice) whose partial results a second kernel folds; the block
 * length only schedules the work: every output is bit-identical for every block length and on every call.  work: device memory of
 * d2d_flight_audit_workspace(p, n_mov) bytes (a negative value: D2D_EINVAL), 16-byte aligned, that the call overwrites.
 * D2D_EINVAL before anything is launched: NULL ctx, p, X_hist, work or out; n_form < 1; n_ac outside 1 .. 64; n_rows < 1; dt_row not
 * > 0; n_stat outside 0 .. D2D_MAX_OBS or n_mov outside 0 .. D2D_MAX_MOV (mov NULL: 0), n_knot out of range; a NULL stat, knots, disc
 * or mov_work with a non-zero count; one of x_ref, y_ref without the other, or a tracking-error output without them; n_mov > 0 without
 * t_start; rows_per_block < 0; err_tol < 0 or NaN.  tests/flight_audit_ref.py is the CPU statement.  Asynchronous on the context's
 * stream. */
#define D2D_AUDIT_NONFINITE 1
#define D2D_AUDIT_BAD_TSTART 2
#define D2D_AUDIT_BAD_TRACK 4
typedef struct {
  int32_t n_form, n_ac;       /* n_ac 1 .. 64 */
  int32_t n_rows;             /* rows of X_hist, x_ref, y_ref and mov_work */
  int32_t rows_per_block;     /* 0: the library's choice */
  int32_t n_stat;             /* 0 .. D2D_MAX_OBS */
  int32_t reserved;
  double dt_row;
  double d_safe;              /* <= 0: no count */
  double err_tol;             /* +inf: no count */
} d2d_audit_params;
typedef struct {
  double *sep_dist; int32_t *sep_partner; double *sep_time; int32_t *sep_count;
  double *stat_clear; double *stat_time; int32_t *stat_count;
  double *mov_clear; double *mov_time; int32_t *mov_count;
  double *err_max; double *err_time; int32_t *err_count;
  double *phi_max; double *v_min; double *v_max;
  int32_t *status;
} d2d_audit_out;
int64_t d2d_flight_audit_workspace(const d2d_audit_params *p, int n_mov);
int d2d_flight_audit(d2d_ctx *ctx, const d2d_audit_params *p, const double *X_hist, const int32_t *rows, const double *t_start,
                     const double *x_ref, const double *y_ref, const double *stat, const d2d_moving_obstacles *mov, double *mov_work,
                     void *work, const d2d_audit_out *out);

/* ---- Wind-field estimation from flown histories (version 122) ---------------------------------------------------------------------
 * Every aircraft of a history is a moving anemometer: ground velocity minus air velocity is the wind at its own position and time.
 * d2d_wind_fit fits the control points of a d2d_wind_field (geometry given by the caller) to a history that is on the device.
 * tests/wind_fit_ref.py is the CPU statement (numpy / scipy.sparse), including the fixed-point rule below, bit for bit.
 *
 * Input.  X_hist dev [n_rows][5][N] (planes x, y, psi, phi, v; N = n_form * n_ac), rows dev int32 [n_form] (NULL: n_rows; clamped to
 * 0 .. n_rows; a row at an index >= rows[f] is never read), t_start dev [n_form] (NULL: 0), dt_row: as in d2d_flight_audit.
 * Measurement.  Two consecutive valid rows i, i + 1 of one drone give one sample (trapezoid rule):
 *   value     m = (p[i+1] - p[i]) / dt_row - 1/2 (v[i] u(psi[i]) + v[i+1] u(psi[i+1])),  u = (cos, sin)
 *   position  1/2 (p[i] + p[i+1]),   time  t_start[f] + (i + 1/2) dt_row.
 * Its error is O(dt_row^2), about dt_row^2 / 12 * v * psidot^2.  psi enters through cos and sin only (its wrap is harmless); both are
 * computed by one fixed sequence of IEEE operations (Cody-Waite reduction by pi/2 in three parts, the fdlibm kernel polynomials,
 * no fused multiply-add; within 2 ulp for |psi| <= 1e6) that the CPU statement repeats, so that m is the same bits on both sides.
 * Rejection, counted by reason, in this order: (1) one of the ten numbers of the two rows (or, with nt > 1, the sample time) is not
 * finite; (2) the midpoint is outside the grid's box [x0, x0 + (nx - 3) hx] x [y0, y0 + (ny - 3) hy] (x [t0, t0 + (nt - 3) ht] when
 * nt > 1) -- rejected, not clamped: clamping would bias the boundary control points; (3) |m_x| or |m_y| > w_max.  The box is closed
 * and so is the limit: a midpoint exactly on an edge is used (s = -0.0 counts as the lower edge; on the upper edge s = n - 3, segment
 * n - 4, r = 1) and so is a sample with |m| = w_max exactly.
 * Unknowns.  c [nt ny nx] per component, nt ny nx <= D2D_WINDFIT_MAX_CP; wx and wy share the design matrix (two right-hand sides).
 * Design row.  The 16 (nt = 1: by[a] bx[b]) or 64 (bt[c] (by[a] bx[b])) tensor-product weights of the sample's cell, with the axis
 * weights of d2d_wind_field (segment i = min(floor(s), n - 4), r = s - i, B_k(r)), evaluated without fused multiply-add.
 * Objective.  sum_s |A_s c - m_s|^2 + lam_x sum (d2_x c)^2 + lam_y sum (d2_y c)^2 + lam_t sum (d2_t c)^2 + mu sum (c - c_prior)^2,
 * d2 the second difference of the control points along an axis (interior points only), c_prior = grid->cp (NULL: 0).  mu > 0 is
 * required: a cell that no aircraft visited is otherwise undetermined.
 * Normal matrix.  H = A^T A is stored by stencil: H_out dev [nt ny nx][S], S = 49 (nt = 1) or 343, entry
 * [p][((dt + 3) 7 + (dy + 3)) 7 + (dx + 3)] (steady: [(dy + 3) 7 + (dx + 3)]) couples p and the point at offset (dt, dy, dx); entries
 * whose partner is outside the grid are 0.  b_out dev [2][nt ny nx] = A^T m.
 * Fixed point, and why every output is independent of the order of the work.  Every product w_i w_j of a sample (in [0, 1]) is
 * rounded to a multiple of 2^-32 (round to nearest even) and every w_i m / W, W = w_max rounded up to a power of two, likewise; the
 * sums are integers: exact in fp64 registers for up to 2^20 samples, then added to the 64-bit stencil storage with integer
 * atomics.  Integer addition is associative and commutative, so H_out, b_out, support, the counts and with them cp_out are bit-identical from call to call, under
 * any permutation of the formations (rows and t_start permuted alike) and for every launch geometry (p->waves): where a wavefront
 * hands its sums over (when its cell changes, at the end of its share) schedules the work and nothing else.  Quantisation: at most
 * 2^-33 per sample and entry of H, 2^-33 W per sample and entry of b.  (n_rows - 1) N < 2^31 keeps every sum below 2^63: beyond,
 * D2D_EINVAL.  H and b of several ranks add exactly in this form.
 * The work is cut into units of D2D_WINDFIT_CHUNK consecutive samples of one drone (one wavefront-load); a wavefront walks its units
 * in time order.  The workspace does not grow with the number of samples.
 * Solve.  (H + penalties + mu I) c = A^T m + mu c_prior for both components by Jacobi-preconditioned conjugate gradients in fp64, one
 * workgroup, every reduction in a fixed order, from c = c_prior, until |r| <= cg_tol |rhs| per component or cg_max iterations.
 * Terminal states.  A component that has met its tolerance is frozen while the other goes on: its control points are the same bits
 * whatever the other component's right-hand side and prior are.  A component whose right-hand side is exactly zero and whose prior
 * is zero is frozen at once, at c = 0, and counts as residual 0.  At the cap cp_out is iterate cg_max (not an error, not the
 * prior): stats[6] == cg_max, and stats[7] > cg_tol is the residual of that iterate (the recursively updated one, which is the true
 * |M c - rhs| / |rhs| of cp_out within about iterations x eps x cond(M)); the caller reads stats to tell.
 * Outputs.  cp_out dev [nt][2][ny][nx]: with the caller's geometry a d2d_wind_field, no host visit.  d2d_windfit_out (any NULL, and
 * out itself may be NULL: cp_out and every member given are the same bits for every selection; a NULL member is not written, and
 * with stats NULL the residual pass is not launched):
 *   support dev [nt ny nx]   diag A^T A in the fixed point below: how much data backs each control point.  A control point whose
 *                            weight stays below 2^-16.5 in every sample has support 0 (each square rounds to 0) though its
 *                            products with larger weights need not vanish: support == 0 does not say that the row of H is zero.
 *                            With lam = 0, cp_out is the prior bit for bit at every control point whose row of H_out is zero.
 *   stats   dev double [8]   samples used; rejected as non-finite, outside the box, above w_max; residual sum of squares of the fitted
 *                            field over the used samples, x and y (a second streaming pass whose partials are folded in a fixed order;
 *                            the RMS residual is about the gust level); CG iterations; largest relative CG residual reached
 *   H_out, b_out             as above
 * A formation with fewer than two valid rows contributes nothing; with no sample at all the answer is the prior (not an error).
 * work: device memory of d2d_wind_fit_workspace(p, grid) bytes (negative: D2D_EINVAL), 16-byte aligned, overwritten: what it holds
 * on entry does not matter (no output depends on it), and nothing is written beyond that size or beyond the sizes of the outputs.
 * D2D_EINVAL before anything is launched: NULL ctx, p, X_hist, grid, cp_out or work; a geometry d2d_wind_sample refuses (grid->cp may
 * be NULL here); nt ny nx > D2D_WINDFIT_MAX_CP; n_rows < 2, n_form < 1, n_ac outside 1 .. 64; dt_row, w_max or mu not > 0 or not
 * finite; a negative or non-finite lam_*; cg_tol not in (0, 1); cg_max < 1; waves < 0; (n_rows - 1) N >= 2^31.  Asynchronous on the
 * context's stream. */
#define D2D_WINDFIT_MAX_CP 4096
#define D2D_WINDFIT_CHUNK 64
typedef struct {
  int32_t n_form, n_ac;       /* n_ac 1 .. 64 */
  int32_t n_rows;             /* rows of X_hist (>= 2) */
  int32_t cg_max;             /* >= 1 */
  int32_t waves;              /* wavefronts of the accumulation launch, 0: the library's choice (schedules only: same bits) */
  int32_t reserved;
  double dt_row;
  double w_max;               /* a sample with a component above it is rejected */
  double lam_x, lam_y, lam_t; /* >= 0 (lam_t is not read when nt = 1) */
  double mu;                  /* > 0 */
  double cg_tol;              /* in (0, 1) */
} d2d_windfit_params;
typedef struct {
  double *support, *stats, *H_out, *b_out;
} d2d_windfit_out;
int64_t d2d_wind_fit_workspace(const d2d_windfit_params *p, const d2d_wind_field *grid);
int d2d_wind_fit(d2d_ctx *ctx, const d2d_windfit_params *p, const double *X_hist, const int32_t *rows, const double *t_start,
                 const d2d_wind_field *grid, double *cp_out, void *work, const d2d_windfit_out *out);

/* ---- Fleet audit: separation between aircraft of DIFFERENT formations (version 123) ----------------------------------------------------
 * d2d_flight_audit looks inside a formation; this call looks across them.  Per aircraft: the closest approach, continuous in time
 * between rows, to any aircraft of another formation that shares its airspace, found through a spatial grid so that the cost grows
 * with the history and not with N^2.  tests/fleet_audit_ref.py is the CPU statement: brute force over all pairs.
 * History.  X_hist dev [n_rows][5][N], N = n_form * n_ac, drone d = formation d / n_ac: the layout of d2d_flight_audit.  Only the x and
 * y planes are read.  rows dev int32 [n_form] (NULL: n_rows; clamped to 0 .. n_rows) is the number of valid rows of each formation: a
 * row at an index >= rows[f] is never read.
 * Common clock.  Formations are compared on integer rows: row0 dev int32 [n_form] (NULL: 0) places row i of formation f at the global
 * row row0[f] + i, and the global rows 0 .. g_rows - 1 are swept.  Formation f is VALID at the global row g when 0 <= g - row0[f] <
 * rows[f].  A reported time is (g + s) dt_row: the caller adds the epoch.  Start times that are not a whole number of rows apart cannot
 * be stated here.
 * Worlds.  world dev int32 [n_form] (NULL: one world): only aircraft of different formations in the SAME world are compared (Monte-Carlo
 * replicas that lie on top of each other get one world each).
 * Candidates and key: those of d2d_flight_audit, by the same device function (csrc/audit_device.h).  For aircraft A and B of different
 * formations and the same world and a global row g at which both are valid, with p = (position of B) - (position of A): the row's own
 * |p0|^2 is a candidate at time g; if both are also valid at g + 1, so is the interior closest approach |p0 + s* d|^2 at g + s* where
 * 0 < s* < 1 (s* = 1 is the next row's own candidate).  The answer of A is the lexicographic minimum of the keys (d^2, g + s, B's global
 * drone index) -- the smallest distance, then the earliest time, then the smallest index -- and the square root is drawn once, at the end.
 * Look radius.  d_look > 0: a candidate counts only when d^2 < d_look^2, strictly.  Nothing within d_look is "nothing seen": distance
 * +inf, partner -1, time NaN, count 0.  The answer is therefore a property of the history alone: it equals the brute-force minimum over
 * all pairs whenever that minimum is below d_look, and the grid below only schedules the search.
 * Step bound.  step_max > 0: no aircraft moves farther than step_max between two consecutive valid rows.  It is checked, not trusted
 * (D2D_FLEET_STEP: dx^2 + dy^2 > step_max^2).  If the closest approach q = p0 + s d of a segment is below d_look then |p0| <= |q| + s |d| <
 * d_look + 2 step_max: at the segment's FIRST row the pair is less than E0 = d_look + 2 step_max apart on either axis.  (E0 is reached
 * only by s = 1, the next row's own candidate; an INTERIOR approach below d_look starts within sqrt(d_look^2 + 4 step_max^2), since
 * q is perpendicular to d there.  The grid keeps the simpler, larger E0; tests/test_gpu_fleet_audit.py places pairs at the interior
 * bound, which an edge of d_look + step_max loses when step_max > 2/3 d_look.)  The grid has
 * square cells of edge E = E0 (1 + 2^-16) and cell index floor(coordinate * (1 / E)) per axis; every valid aircraft is binned at every
 * row, and an aircraft looks into its own cell and the eight around it.  Rounding cannot lose a pair: a formation with a coordinate
 * whose |coordinate * (1 / E)| exceeds 2^30 is refused (D2D_FLEET_RANGE), so a computed quotient is within 2^30 * 3 * 2^-53 < 2^-21 of the
 * true one, while two coordinates less than E0 apart have true quotients less than 1 / (1 + 2^-16) < 1 - 2^-17 apart: the computed
 * quotients differ by less than 1 and their floors by at most 1.  The roundings of the step check and of d^2 < d_look^2 move E0 by a
 * few parts in 2^53 and disappear in the same margin.
 * Outputs (d2d_fleet_out; any pointer may be NULL: not stored):
 *   near_dist, near_time   double [N]  the closest approach to an aircraft of another formation and its time (g + s) dt_row
 *   near_partner           int32 [N]   that aircraft's global drone index
 *   near_count             int32 [N]   the global rows at which the nearest other-formation aircraft AT THE ROW is closer than d_safe
 *                                      (d_safe <= 0: no count, 0; d_safe > d_look: D2D_EINVAL, the grid would not see every such row)
 *   status                 int32 [n_form]  0, or the D2D_FLEET_* bits of a refusal
 * Refusals, per formation, decided by a first pass over the x and y planes before anything is compared (the conditions are evaluated
 * independently, so bits can come together: an infinite coordinate is NONFINITE and RANGE):
 *   D2D_FLEET_NONFINITE  a non-finite x or y in a valid row          D2D_FLEET_STEP   a step between two valid rows longer than step_max
 *   D2D_FLEET_BAD_ROW0   row0[f] < 0 or row0[f] + rows[f] > g_rows   D2D_FLEET_RANGE  |coordinate / E| > 2^30 in a valid row
 * A refused formation has NaN floating outputs and -1 counts and partners, and it is invisible to every other formation: those are
 * audited as if it were absent.
 * Scheduling.  The global rows are binned tile_rows at a time (0: the library's choice, a function of N alone; at most 32768); per binned row a hash table of
 * `slots` list heads (0: the library's choice; rounded up to a power of two, at most 2^24) keyed by (world, cell) holds the valid
 * aircraft as linked lists, built with one integer exchange per aircraft.  Cells that share a slot cost a second look and nothing else
 * (slots = 1 compares every aircraft with every other: brute force on the device).  Each (aircraft, row) of a tile is searched by one
 * lane, and one lane per aircraft folds the tile's keys into the aircraft's running key in ascending row order.  The fold is a minimum
 * of keys and the count an integer sum: no floating-point atomic, no floating-point sum, and the order in which a list was built is
 * not seen.  Every output is bit-identical for every tile_rows and slots and from call to call.
 * work: device memory of d2d_fleet_audit_workspace(p) bytes (negative: D2D_EINVAL), 16-byte aligned, overwritten; its size depends on N,
 * tile_rows and slots, not on n_rows.
 * D2D_EINVAL before anything is launched: NULL ctx, p, X_hist, work or out; n_form < 1; n_ac outside 1 .. 64; n_rows < 1; g_rows < 1;
 * dt_row, d_look or step_max not > 0 or not finite; d_safe > d_look (or NaN); tile_rows < 0 or slots < 0; a history or a tile too large
 * to index (N >= 2^31, 5 N n_rows >= 2^40, N tile_rows >= 2^31).  Asynchronous on the context's stream. */
#define D2D_FLEET_NONFINITE 1
#define D2D_FLEET_STEP 2
#define D2D_FLEET_BAD_ROW0 4
#define D2D_FLEET_RANGE 8
typedef struct {
  int32_t n_form, n_ac;       /* n_ac 1 .. 64 */
  int32_t n_rows;             /* rows of X_hist */
  int32_t g_rows;             /* global rows swept */
  int32_t tile_rows;          /* global rows binned per pass, 0: the library's choice (schedules only: same bits) */
  int32_t slots;              /* list heads per binned row, 0: the library's choice (schedules only: same bits) */
  double dt_row;
  double d_look;              /* > 0 */
  double step_max;            /* > 0 */
  double d_safe;              /* <= 0: no count; <= d_look */
} d2d_fleet_params;
typedef struct {
  double *near_dist; int32_t *near_partner; double *near_time; int32_t *near_count;
  int32_t *status;
} d2d_fleet_out;
int64_t d2d_fleet_audit_workspace(const d2d_fleet_params *p);
int d2d_fleet_audit(d2d_ctx *ctx, const d2d_fleet_params *p, const double *X_hist, const int32_t *rows, const int32_t *row0,
                    const int32_t *world, void *work, const d2d_fleet_out *out);

/* ---- Fleet tracks: the aircraft a formation must give way to, as moving-obstacle tables (version 125) -------------------------------------
 * d2d_fleet_audit says who came near whom; this call turns the same search into the input of a re-plan.  Formations are ranked by the
 * pair (prio[f], f), smaller first (prio dev int32 [n_form]; NULL: the formation index): the formation with the smaller pair keeps its
 * plan, the other one gives way.  For every formation f the call writes the tracks of the nearest aircraft that OUTRANK it, in the
 * layout of d2d_moving_obstacles with G = n_form, ready for d2d_nlp_solve_groups_moving (R = n_form) or d2d_nlp_solve_moving (n_ac = 1).
 * tests/fleet_tracks_ref.py is the CPU statement: brute force over all pairs.
 * History, clock, worlds, look radius, step bound, refusals, scheduling: the arguments of d2d_fleet_audit with the same meanings
 * (p->d_safe is not used beyond its rule d_safe <= d_look).
 * Definition -- a property of the history alone.  C(f) holds every aircraft B of another, non-refused formation of f's world whose
 * (prio, formation) is smaller than f's and for which some aircraft A of f and some candidate of the audit (a row's own distance, or an
 * interior closest approach between two rows: csrc/audit_device.h) has d^2 < d_look^2, strictly.  The key of B is the lexicographic
 * minimum over those A and candidates of (d^2, g + s, A's global index).  C(f) is ordered by (key, B's global index) and its first n_mov
 * members are written, member m to slot m.
 * Outputs (d2d_tracks_out; any pointer may be NULL: not stored):
 *   knots      double [n_form][n_mov][n_knot][3] = (t, x, y).  Knot k of formation f lies at the global row
 *              g_k = row0[f] + (k (rows[f] - 1)) / (n_knot - 1) (integer division: knot 0 at f's first row, the last knot at its last),
 *              at the time t0 + g_k dt_row (the product rounded, then the sum: one multiply and one add, not accumulated; t0 is the time
 *              of global row 0), at B's own history values at its local row clamp(g_k - row0[B's formation], 0, rows[B's formation] - 1):
 *              a partner outside its own window is held at its first or last row, as the table holds a track outside its knots.
 *   disc       double [n_form][n_mov][2] = (r_disc, kind); an absent slot (fewer than n_mov members) has r = 0, the same kind, and a
 *              valid dummy track: the knot times above, positions 0 (the solve kernels validate absent discs too).
 *   partner    int32 [n_form][n_mov]   B's global drone index, -1: absent
 *   part_dist, part_time  double [n_form][n_mov]  the root of the key's d^2, drawn once at the end, and (g + s) dt_row; absent: +inf, NaN
 *   chord_err  double [n_form][n_mov]  what the decimation to n_knot knots gives away: the largest distance, over the global rows g of
 *              f's window at which B has a row of its own, between B's position at that row and the written track at the row's time.
 *              With k the largest index <= n_knot - 2 with g_k <= g and (xa, ya), (xb, yb) the written knots k and k + 1:
 *              s = (g - g_k) / (g_k+1 - g_k), p = a + s (b - a), e^2 = (x - px)^2 + (y - py)^2, every operation rounded on its own (nothing
 *              fused), the maximum of e^2 over the rows exact, the root drawn once.  Absent: 0.  The caller adds it to r_disc.
 *   n_conf     int32 [n_form]   min(|C(f)|, n_mov + 1): the value n_mov + 1 says "more partners than slots"
 *   status     int32 [n_form]   the D2D_FLEET_* bits, plus D2D_TRACKS_SHORT when rows[f] (clamped) < n_knot: the knot times would not
 *              increase strictly
 * A formation with a non-zero status has n_conf = -1, partners -1, NaN floating outputs, absent discs and dummy tracks with one knot per
 * row from row0[f] (times t0 + (row0[f] + k) dt_row, positions 0).  A formation refused by a D2D_FLEET_* bit is invisible to the others;
 * one that is only D2D_TRACKS_SHORT has a sound history and is seen.
 * Every output is bit-identical for every tile_rows and slots (slots = 1: brute force on the device) and from call to call: the
 * n_mov + 1 smallest distinct partners, each with the minimum of its keys, are kept through a merge that is commutative and
 * associative; a member of the final list cannot be lost on the way, since fewer than n_mov + 1 others ever stand before it.  No
 * floating-point atomic, no floating-point sum.
 * work: device memory of d2d_fleet_tracks_workspace(p, n_mov) bytes (negative: D2D_EINVAL), 16-byte aligned, overwritten; its size
 * depends on N, tile_rows, slots and n_mov, not on n_rows.
 * D2D_EINVAL before anything is launched: the rules of d2d_fleet_audit; n_mov outside 1 .. D2D_MAX_MOV; n_knot outside 2 ..
 * D2D_MOV_MAX_KNOT; r_disc not > 0 or not finite; kind neither 0 nor 1; t0 not finite.  Asynchronous on the context's stream. */
#define D2D_TRACKS_SHORT 16
typedef struct {
  double *knots; double *disc; int32_t *partner; double *part_dist; double *part_time; double *chord_err;
  int32_t *n_conf; int32_t *status;
} d2d_tracks_out;
int64_t d2d_fleet_tracks_workspace(const d2d_fleet_params *p, int n_mov);
int d2d_fleet_tracks(d2d_ctx *ctx, const d2d_fleet_params *p, const double *X_hist, const int32_t *rows, const int32_t *row0,
                     const int32_t *world, const int32_t *prio, int n_mov, int n_knot, double r_disc, int kind, double t0, void *work,
                     const d2d_tracks_out *out);

/* ---- the start of a collocation solve from a Dubins path (version 124) ----
 * d2d_nlp_guess_dubins fills W [B][5][N] with node values (x, y, psi, phi, v) that are almost a feasible point of the collocation
 * NLP of d2d_nlp_solve and its family: circular arcs at the fraction kappa of the bank limit joined by a straight line or a third
 * arc, flown at ONE speed, in the air frame of the row's constant wind.  tests/nlp_guess_ref.py is the CPU statement; the kernel
 * follows it decision for decision (DESIGN 5.23 has the rule in words).  Per problem, from its scenario row as nlp_load_scen reads it:
 *   end poses p0, p1 (D2D_SC_X0 .. PSI1); the drift w = (D2D_SC_WX, D2D_SC_WY) of the solver's equalities x' = v cos psi + w_x;
 *   v_lo, v_hi = D2D_SC_VMIN, VMAX; phi_max = D2D_SC_PHIMAX, or min(|phi_lo|, |phi_hi|) of opts->bounds where phi_lo < phi_hi;
 *   v_pref = opts->v_pref[b], or with v_pref NULL: D2D_SC_VSP where D2D_SC_KV > 0, else D2D_SC_VREF where > 0, else (v_lo + v_hi) / 2;
 *   clamped into [v_lo, v_hi].
 * T = (N - 1) h; the path runs from p0 to p1' = (x1 - w_x T, y1 - w_y T, psi1) and node i is shifted by w i h.  Turn radius
 * rho(v) = v^2 / (g tan(kappa phi_max)).  Of the six words LSL, RSR, LSR, RSL, RLR, LRL (the word index, in this order) only those
 * whose NET TURNING equals psi1 - psi0 to D2D_GUESS_TURN_TOL are admissible -- the NLP pins psi at both ends as numbers, not modulo
 * 2 pi -- and L*(rho) is the shortest admissible length (+inf: none; ties to the lower index).  F(v) = L*(rho(v)) - v T.
 *   F(v_pref) > 0, the duration is tight: v in [v_pref, v_hi] with F = 0 (D2D_GUESS_FIT), or v = v_hi where F(v_hi) > 0
 *     (D2D_GUESS_SHORT: the path is longer than v_hi T and is sampled by arc-length fraction all the same).
 *   F(v_pref) <= 0, loose: v = v_pref and rho >= rho(v_pref) with L*(rho) = v T (D2D_GUESS_LOOSE); the bracket grows by factors of
 *     D2D_GUESS_GROW at most D2D_GUESS_GROW_MAX times; never reached: the last radius (D2D_GUESS_LOOSE_UNMET).
 *   The search: D2D_GUESS_ROUNDS rounds of 64-section -- the 63 interior points a + (b - a) k / 64 of the bracket, the first
 *   sub-interval from the lower end whose ends are on different sides (the bracket's own ends keep the sides they had).  The result
 *   is the upper end of the last speed bracket and the LOWER end of the last radius bracket: the side where L* <= v T.  L* can jump
 *   (a word stops existing or being admissible); the search still ends on that side, and L then falls short of v T.
 * Node i lies at arc length L i / (N - 1) (a node on a junction belongs to the earlier segment); phi = +- atan(v^2 / (g rho)) on a
 * left / right arc, 0 on the straight; v constant; nodes 0 and N - 1 carry the end poses as the numbers of the row.
 * D2D_GUESS_LINE: |psi1 - psi0| >= 2 pi, no admissible word, or L* = 0 -- x, y, psi linear between the ends, phi = 0, v = v_pref.
 * D2D_GUESS_INVALID: a non-finite entry among those read, v_lo <= 0, v_lo > v_hi, phi_max outside (0, pi/2): W of the row is NOT
 * written, word = -1, v = rho = L = t_nat = NaN.
 * Outputs (d2d_nlp_guess_out; the struct or any pointer may be NULL: not stored): status, word (-1: LINE / INVALID) int32 [B];
 * v, rho (+inf: LINE), L (the path's length in the air frame; LINE: the ground distance), t_nat double [B].
 * t_nat = L*(rho(v_pref)) / v_pref (NaN: no admissible word there) is the duration at which the preferred speed flies the shortest
 * path: a SUGGESTION for the start step of d2d_nlp_solve_free, h = t_nat / (N - 1).  It is NOT a lower bound on the duration: a
 * slower aircraft turns tighter, and problems whose t_nat exceeds T by several per cent converge at T.
 * Not done here (refuse upstream): paths round static, moving or keep-out discs or through pins, spatial wind fields (the row's
 * constant wind is used), loops for durations that no widened turn fills.
 * D2D_EINVAL before anything is launched: NULL ctx, scen or W; B < 1; N < 2; h not > 0 or not finite; kappa outside (0, 1].
 * opts NULL: kappa = D2D_GUESS_KAPPA, no bounds, no v_pref.  Asynchronous on the context's stream; one owner per output, no atomics:
 * the same bytes from call to call and for every grid (opts->waves, 0: the library's choice; scheduling only). */
#define D2D_GUESS_FIT 0
#define D2D_GUESS_SHORT 1
#define D2D_GUESS_LOOSE 2
#define D2D_GUESS_LOOSE_UNMET 3
#define D2D_GUESS_LINE 4
#define D2D_GUESS_INVALID 5
#define D2D_GUESS_KAPPA 0.9
#define D2D_GUESS_TURN_TOL 1e-9
#define D2D_GUESS_ROUNDS 3
#define D2D_GUESS_GROW 1.5
#define D2D_GUESS_GROW_MAX 24
typedef struct {
  double kappa;           /* fraction of the bank limit the arcs use, in (0, 1] (D2D_GUESS_KAPPA) */
  const double *bounds;   /* dev [B][4] as d2d_nlp_opts.bounds, or NULL */
  const double *v_pref;   /* dev [B], or NULL */
  int32_t waves;          /* wavefronts of the launch, 0: the library's choice (schedules only: same bytes) */
  int32_t reserved;
} d2d_nlp_guess_opts;
typedef struct {
  int32_t *status; int32_t *word;
  double *v; double *rho; double *L; double *t_nat;
} d2d_nlp_guess_out;
int d2d_nlp_guess_dubins(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_guess_opts *opts, double *W,
                         const d2d_nlp_guess_out *out);

/* Gust dispersion of a tracked plan: the covariance of the deviation that d2d_sim_track_run_gust's flight shows from the gust-free flight
 * of the same references, predicted by ONE deterministic pass per plan -- no sampling.  The tracking loop is a linear feedback round a
 * known reference whose gain depends on the reference alone (ComputeGain evaluates cont_jac and the Riccati equation at Xr), and the
 * gust g = w_own o + w_form h is, per axis, one first-order Gauss-Markov process of variance sigma^2 (w_own^2 + w_form^2 = 1) held over a
 * step.  Deviation state of a drone: z = (dx, dy, dpsi, dphi, dv, gx, gy), covariance S (7 x 7).
 *   Start     S_0 = blockdiag(P0 or 0_5, sigma^2 I_2): S_in, or without one the stationary start of the loops without state_in.
 *   Step i = 1 .. n_rows - 1, with reference sample i as the tracking loop pairs them (derivatives: its two passes of
 *   numpy.gradient(edge_order=2) / dt; n_rows = 2: the one first difference, the second derivative 0):
 *     Xr_i, K_i (2 x 5)  those of d2d_ctrl_gain at X = Xr_i -- the same flatness map, cont_jac with its quirk entries, the CARE, Yddd = 0;
 *     A_i     the TRUE Jacobian of the plant's equations of motion at (psi, phi, v) = Xr_i: cont_jac's rows 0, 1, 3, 4 and
 *             d psi'/d phi = g / (v cos^2 phi), d psi'/d v = -g tan phi / v^2;  B = [0; 0; 0; 1/tau_phi, 0; 0, 1/tau_v];
 *             E = d f / d w: ones in rows 0 and 1;
 *     [Ad Bd Ed] = the first five rows of expm(dt [[A B E], [0 0 0]]) (9 x 9): input and gust are zero-order holds over the step
 *             (evaluated in closed form: the phi and v lags are decoupled, psi and (x, y) are integrals of their exponentials);
 *     F_i = [[Ad - Bd K_i, Ed], [0, a I_2]],   S_i = F_i S_{i-1} F_i^T + diag(0_5, s^2, s^2).
 *   The error saturations, phi_lim, v_min / v_max and the wrap of psi are ignored: that is the approximation.  p->n_rows, dt, tau_phi,
 *   tau_v, wx, wy, q_diag, r_diag are read as d2d_sim_track_run reads them; x_ref, y_ref dev [n_rows][n].
 * in:   a, s, sigma of d2d_gust; S_in dev [28][n] or NULL.  S is stored as its packed lower triangle, entry (i, j), i >= j, at
 *       i (i + 1) / 2 + j, plane-major across drones.
 * out (any pointer may be NULL: not stored), Ppos_i = S_i[0:2, 0:2]:
 *   Ppos_hist dev [n_rows][3][n] = xx, xy, yy: row i pairs with X_hist row i of the flight (row 0: the start);  S_out dev [28][n]: S after
 *   the last row (a call that continues with S_in = S_out from the LAST row of this one reproduces one long call where the references'
 *   derivatives agree);
 *   sig_max [n] = max_i sqrt(lambda_max(Ppos_i)) and sig_row, its row;
 *   per edge e = (ax, ay, b, .) of fence->edges [n][n_edge][4] (kap is not read; ax = ay = 0: absent):
 *     fence_sn [n_edge][n] = max_i sqrt(a^T Ppos_i a),  fence_k = min_i (b - a . p_ref_i) / sqrt(a^T Ppos_i a)  and fence_row, its row;
 *   per disc (cx, cy, R) of keep->discs [n][n_keep][3] (R <= 0: absent):
 *     disc_k [n_keep][n] = min_i (|p_ref_i - c| - R) / sqrt(u^T Ppos_i u), u the unit vector from the centre, and disc_row, its row.
 *   The reductions run over i >= 1 and keep the first row of an extreme; a zero variance gives k = +inf (every row: row 1); an absent
 *   row gives fence_sn = 0, k = +inf, row -1.  fence_k / fence_row and disc_k / disc_row are given together.
 * D2D_EINVAL before any launch: a NULL in or out; n < 1 or n_rows < 2; a outside [0, 1); s or sigma negative or not finite; n_edge
 * beyond D2D_MAX_FENCE or n_keep beyond D2D_MAX_KEEP, a count > 0 with a NULL table; a fence or disc output without its table (fence or
 * keep NULL, or a count of 0).  fence, keep may be NULL.  One drone per lane and no exchange between lanes in the new arithmetic: a
 * drone's result does not depend on the batch beyond what d2d_ctrl_gain's Riccati solver already shares with its wavefront.
 * tests/dispersion_ref.py is the CPU statement.  Asynchronous on the context's stream.  (version 128) */
typedef struct {
  double a, s, sigma;   /* exp(-dt / tau), sigma sqrt(1 - a^2), sigma (m/s): d2d_gust's */
  const double *S_in;   /* dev [28][n] or NULL */
} d2d_dispersion_in;
typedef struct {
  double *Ppos_hist;    /* dev [n_rows][3][n] = xx, xy, yy, or NULL */
  double *S_out;        /* dev [28][n] or NULL */
  double *sig_max; int32_t *sig_row;                        /* dev [n] */
  double *fence_sn; double *fence_k; int32_t *fence_row;    /* dev [n_edge][n] */
  double *disc_k; int32_t *disc_row;                        /* dev [n_keep][n] */
} d2d_dispersion_out;
int d2d_track_dispersion(d2d_ctx *ctx, const d2d_track_params *p, const double *x_ref, const double *y_ref,
                         const d2d_dispersion_in *in, const d2d_fence *fence, const d2d_keep_out *keep, const d2d_dispersion_out *out);

#ifdef __cplusplus
}
#endif
#endif /* D2D_H */
