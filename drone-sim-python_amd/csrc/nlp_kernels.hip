// Direct-collocation NLP of the reference's planners in its own parameterisation -- node values (x, y, psi, phi, v)(t_i),
// backward-Euler collocation equalities, end conditions, HARD box bounds -- solved on the device: the backend that stands
// where the reference builds `opty.direct_collocation.Problem(...)` and calls `.solve(x0)` (IPOPT)
// (src/single_opt_planner.py:62-71,124; src/multi_opt_planner.py:69-78,86).  The algorithm is oracle/nlp.py's, step for step:
//   equalities  -> augmented Lagrangian (scaled multiplier estimate mu, penalty rho)
//   bounds      -> primal-dual log barrier (parameter mub, duals zL / zU), fraction-to-the-boundary rule
//   inner step  -> damped Newton on the block-tridiagonal system  H/2 + Sigma/2 + lam |diag|  (Lagrangian Hessian incl. the
//                  constraint curvature), backtracking line search on the barrier-AL merit function
// (the oracle solves that system with banded LAPACK; here: per-node elimination of phi, v + 3x3 block Cholesky, see below).
// One problem per WAVEFRONT.  Everything that is independent from node to node -- merit function, assembly of the Hessian
// blocks, ratio tests, the update -- runs with lane = node (chunks of 64, DPP reductions); only the two block recursions
// (Cholesky + forward substitution, back substitution) are serial in the nodes and run wave-uniform with the next node's
// inputs requested a node ahead.  Per-problem data lives in planes of N doubles ([component][node]: coalesced for lane = node,
// one broadcast request for the serial recursions); control flow is uniform, so no problem waits for another one's line search.
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "fit_device.h"      // scenario row columns (D2D_SC_*), FIT_G, FIT_OBS_K
#include "wind_device.h"     // wind_at, wind_eval2 (d2d_nlp_solve_wind)

#define NLP_NV 5
#ifndef NLP_WIND_NEXT_SHUFFLE
#define NLP_WIND_NEXT_SHUFFLE 1    // (A/B: -DNLP_WIND_NEXT_SHUFFLE=0 evaluates the field at the next node a second time)
#endif

// ---- the feature set of an instantiation ------------------------------------------------------------------------------------
// nlp_merit, nlp_assemble, nlp_recover_stats, nlp_apply, nlp_solve_one, the loop bodies nlp_handout_body and nlp_groups_body and their
// helpers take ONE template argument, the set F of these bits, named at the call: nlp_solve_one<NLP_WIND * WIND | NLP_KEEP | NLP_FENCE>.
//   MODEL (d2d_nlp_solve_model): the objective is the quadratic model ex.md on top of the row's structured terms; cost = its value.
//   WIND  (d2d_nlp_solve_wind): the equalities read the field ex.wf at node i's own (t_start + i h, x_i, y_i), not the row's constant.
//   PAIRS (d2d_nlp_solve_groups_pairs): partner is the scenario's W and ex.pmask this aircraft's partner set (nlp_exp_terms); 0: none.
//   MOV   (d2d_nlp_solve_moving, _groups_moving): ex.mv the soft moving discs (nlp_exp_terms), centre planes sampled at the node times.
//   VIA   (d2d_nlp_solve_via, _groups_via): ex.via the pins, checked by the caller (nlp_via_bad): a pinned component starts at its value
//         and stays there -- no duals, no barrier, no step, an identity row in the Newton system -- exactly as x, y, psi of the two end
//         nodes do.  The terms of the objective still count at a pinned node.
//   FREE  (d2d_nlp_solve_free): h is the problem's own unknown in the box of ex.free_row, started from the row's value or the launch's h;
//         the Newton system is bordered by the row of u = 1 / h (nlp_assemble, nlp_recover_free), every pass reads the equalities at the
//         current u, the line search at the trial one, and cost carries the duration term.  An unusable row of the box refuses the
//         problem like an unusable scenario row; *ex.h_out gets the solved h (NaN for a refused problem).
//         FREE with KEEP and FENCE (d2d_nlp_solve_free_fence): the static hard discs and the half-planes beside the free step.  Both read
//         (x, y) of the interior nodes alone, so the border column b, the scalar d and the residual of the row of u gain no term: what the
//         families add sits in A, and with it in both solves of the Schur complement.  FREE with FENCE brings KEEP (either count may be 0).
//   KEEP  (d2d_nlp_solve_keepout): ex.keep the hard discs and the planes of their duals; g > 0 is held at every interior node by the
//         box's primal-dual barrier (the four passes), the start is moved out of the discs (nlp_keep_start) and unusable discs refuse
//         the problem (nlp_keep_bad).  cost does not see the discs.  KMOV brings KEEP with it.
//   KMOV  (d2d_nlp_solve_keepout_moving, _groups_keepout): ex.keep a NlpKeepMovSet, discs that move: g at node i is taken with the disc's
//         centre at that node's time.  Nothing else changes: the centres are data.
//   FENCE (d2d_nlp_solve_fence, _groups_fence): ex.keep a NlpKeepFenceSet, whose fence holds the half-planes and the planes of their
//         duals; g > 0 is held like the discs', the start is moved inside (nlp_fence_start, behind nlp_keep_start), unusable edges refuse
//         the problem (nlp_fence_bad).  With KEEP the static hard discs are held too; alone (the group kernel) keep is not read.
//   T_AT  (nlp_handout_body alone): the start time is the problem's own, t_at [B] in device memory, read and checked per problem.
constexpr unsigned NLP_MODEL = 1u << 0, NLP_WIND = 1u << 1, NLP_PAIRS = 1u << 2, NLP_MOV = 1u << 3, NLP_VIA = 1u << 4, NLP_FREE = 1u << 5,
                   NLP_KEEP = 1u << 6, NLP_KMOV = 1u << 7, NLP_FENCE = 1u << 8, NLP_T_AT = 1u << 9;
template <unsigned F> struct NlpFeatures {
  static constexpr bool MODEL = (F & NLP_MODEL) != 0, WIND = (F & NLP_WIND) != 0, PAIRS = (F & NLP_PAIRS) != 0, MOV = (F & NLP_MOV) != 0,
                        VIA = (F & NLP_VIA) != 0, FREE = (F & NLP_FREE) != 0, KMOV = (F & NLP_KMOV) != 0, KEEP = KMOV || (F & NLP_KEEP) != 0,
                        FENCE = (F & NLP_FENCE) != 0, T_AT = (F & NLP_T_AT) != 0;
  static_assert(F < (NLP_T_AT << 1), "unknown feature bit");
  static_assert(!MODEL || F == NLP_MODEL, "MODEL excludes every other feature");
  static_assert(!FREE || !(WIND || MOV || VIA || KMOV), "FREE excludes WIND, MOV, VIA and KMOV");
  static_assert(!(FREE && FENCE) || KEEP, "FREE with FENCE brings KEEP, as the fence kernel does (either count may be 0)");
  static_assert(!(KEEP || FENCE) || !(MOV || VIA), "KEEP, KMOV and FENCE exclude MOV and VIA: their problem types carry no soft discs or pins");
  static_assert(!(KMOV && FENCE), "FENCE holds static hard discs only");
};
#define NLP_FEATURES(F)   /* the members of NlpFeatures<F> under their own names, for a function body */                                                \
  [[maybe_unused]] constexpr bool MODEL = NlpFeatures<F>::MODEL, WIND = NlpFeatures<F>::WIND, PAIRS = NlpFeatures<F>::PAIRS, MOV = NlpFeatures<F>::MOV, VIA = NlpFeatures<F>::VIA, \
                                  FREE = NlpFeatures<F>::FREE, KEEP = NlpFeatures<F>::KEEP, KMOV = NlpFeatures<F>::KMOV, FENCE = NlpFeatures<F>::FENCE, T_AT = NlpFeatures<F>::T_AT

// per-problem scenario constants in registers
struct NlpScen {
  double p0[3], p1[3];
  double skv, skphi, vsp, wx, wy;            // s*kv, s*kphi (s = obj_scale / N [/ n_ac]); wind as it enters the eom (+w)
  double sbank;                              // CostBank(use_mean=False): obj_scale * kbank of the term sbank * max_i phi_i^2 (skphi = 0 then); 0 = mean mode
  double lo[NLP_NV], hi[NLP_NV];             // box (+-1e300: open)
  double wobs, wcol, kc2;                    // s*kobs, scol*kcol, (k / rcol)^2
  int n_obs, okind;
};

__device__ __forceinline__ NlpScen nlp_load_scen(const double *__restrict__ sc, const d2d_nlp_opts &o, const double *__restrict__ bnd) {
  NlpScen s;
  s.p0[0] = sc[D2D_SC_X0]; s.p0[1] = sc[D2D_SC_Y0]; s.p0[2] = sc[D2D_SC_PSI0];
  s.p1[0] = sc[D2D_SC_X1]; s.p1[1] = sc[D2D_SC_Y1]; s.p1[2] = sc[D2D_SC_PSI1];
  const double ss = sc[D2D_SC_S];
  s.skv = ss * sc[D2D_SC_KV]; s.skphi = ss * sc[D2D_SC_KPHI]; s.vsp = sc[D2D_SC_VSP];
  s.sbank = 0.0;                             // (nlp_solve_one sets it for D2D_SC_BANKMAX rows: it needs the node count)
  s.wx = -sc[D2D_SC_WX]; s.wy = -sc[D2D_SC_WY];      // the row stores -w (planner convention, single_opt_planner.scen_row)
  s.lo[0] = -1e300; s.hi[0] = 1e300; s.lo[1] = -1e300; s.hi[1] = 1e300; s.lo[2] = -1e300; s.hi[2] = 1e300;
  if (sc[D2D_SC_XMIN] < sc[D2D_SC_XMAX]) { s.lo[0] = sc[D2D_SC_XMIN]; s.hi[0] = sc[D2D_SC_XMAX]; }
  if (sc[D2D_SC_YMIN] < sc[D2D_SC_YMAX]) { s.lo[1] = sc[D2D_SC_YMIN]; s.hi[1] = sc[D2D_SC_YMAX]; }
  s.lo[3] = -sc[D2D_SC_PHIMAX]; s.hi[3] = sc[D2D_SC_PHIMAX];
  s.lo[4] = sc[D2D_SC_VMIN]; s.hi[4] = sc[D2D_SC_VMAX];
  if (bnd) {                                           // d2d_nlp_opts.bounds: an asymmetric phi interval, a box on psi
    if (bnd[0] < bnd[1]) { s.lo[3] = bnd[0]; s.hi[3] = bnd[1]; }
    if (bnd[2] < bnd[3]) { s.lo[2] = bnd[2]; s.hi[2] = bnd[3]; }
  }
  s.wobs = ss * sc[D2D_SC_KOBS];
  const double kcol = sc[D2D_SC_KCOL], rcol = sc[D2D_SC_RCOL];
  s.wcol = (kcol > 0.0 && rcol > 0.0) ? sc[D2D_SC_SCOL] * kcol : 0.0;
  s.kc2 = rcol > 0.0 ? (FIT_OBS_K / rcol) * (FIT_OBS_K / rcol) : 0.0;
  s.okind = (int)sc[D2D_SC_OKIND];
  int n = 0;
  for (int i = 0; i < D2D_MAX_OBS; ++i) {
    const double r = sc[(i < 2 ? D2D_SC_O0R + 3 * i : D2D_SC_OEXT + 3 * (i - 2) + 2)];
    if (r > 0.0) n = i + 1;
  }
  s.n_obs = n;
  (void)o;
  return s;
}

__device__ __forceinline__ void nlp_obs(const double *__restrict__ sc, int i, double &cx, double &cy, double &r) {
  const int c = i < 2 ? D2D_SC_O0X + 3 * i : D2D_SC_OEXT + 3 * (i - 2);
  cx = sc[c]; cy = sc[c + 1]; r = sc[c + 2];
}

// position-dependent exp terms of one node (oracle/nlp.py _obst_terms): adds the objective value (the function whose
// gradient is the reference's cost_grad: kind-1 terms scaled by (r/k)^2), its half gradient and half Gauss-Newton block;
// cost_ref accumulates the reference's cost() value of the same terms.
// PAIRS (d2d_nlp_solve_groups_pairs): `partner` is the base of the scenario's W ([n_ac][5][N], pstride = N) and pmask the set of
// this aircraft's partners, bit j = aircraft j: a wave-uniform value (scalar register), walked bit by bit in a ROLLED loop -- one
// partner's terms live at a time, whatever the count (an unrolled loop over seven partners would spill: the kernel already sits at
// the register limit), and no lane diverges.  Ascending j: with the mask of one partner the sums are the frozen partner's above.
// MOV (d2d_nlp_solve_moving, d2d_nlp_solve_groups_moving): mv holds the problem's moving discs -- centre planes ctr [n][2][N] that
// nlp_mov_sample_kernel wrote ahead of the solve (disc m's x at node i: ctr[(2 m) * N + i], read like a partner's plane) and the table
// disc [n][2] = (r, kind), wave-uniform.  Each disc adds the static disc's term of its kind with the node's own centre, in a rolled
// loop like the partner set's, ascending m, after the static discs and before the partners.
struct NlpMovSet {
  const double *ctr;
  const double *disc;
  int n;
};
template <unsigned F>
__device__ __forceinline__ void nlp_exp_terms(const NlpScen &s, const double *__restrict__ sc, const double *__restrict__ partner,
                                              long pidx, long pstride, double x, double y, double &obj, double &cost_ref, unsigned pmask,
                                              const NlpMovSet *mv, double *gx = nullptr, double *gy = nullptr, double *dxx = nullptr,
                                              double *dxy = nullptr, double *dyy = nullptr) {
  NLP_FEATURES(F);
  for (int i = 0; i < s.n_obs; ++i) {
    double cx, cy, r;
    nlp_obs(sc, i, cx, cy, r);
    if (!(r > 0.0)) continue;
    const double dx = x - cx, dy = y - cy;
    double k2, w, e, f;
    if ((s.okind >> i) & 1) {       // kind 0: e = clip(exp(r^2 - d^2), 0, 1e3) in cost AND in cost_grad = -2 dx e (src/d2d/opty_utils.py:108-131):
      k2 = 1.0; w = s.wobs;         // on the clip that is the gradient of 1e3 (1 + arg - log 1e3), not of the constant cost -- the
      const double arg = r * r - (dx * dx + dy * dy);      // objective minimised continues the term that way (oracle/nlp.py _obst_terms)
      e = exp(fmin(arg, 6.907755278982137));
      f = arg > 6.907755278982137 ? 1e3 * (1.0 + arg - 6.907755278982137) : e;
      cost_ref += w * e;
    } else {                        // kind 1: e = exp(-|k (p - c) / r|^2); cost_grad omits (k/r)^2 (:118-131)
      k2 = (FIT_OBS_K / r) * (FIT_OBS_K / r);
      e = exp(-(dx * dx + dy * dy) * k2);
      cost_ref += s.wobs * e;
      w = s.wobs / k2;
      f = e;
    }
    const double we = w * e;
    obj += w * f;
    if (gx) {
      *gx += -k2 * we * dx; *gy += -k2 * we * dy;
      *dxx += k2 * k2 * we * dx * dx; *dxy += k2 * k2 * we * dx * dy; *dyy += k2 * k2 * we * dy * dy;
    }
  }
  if constexpr (MOV) {
    const double *__restrict__ ctr = mv->ctr, *__restrict__ disc = mv->disc;
#pragma clang loop unroll(disable)
    for (int m = 0; m < mv->n; ++m) {
      const double r = disc[2 * m];
      if (!(r > 0.0)) continue;
      const double dx = x - ctr[(long)(2 * m) * pstride + pidx], dy = y - ctr[(long)(2 * m + 1) * pstride + pidx];
      double k2, w, e, f;
      if (disc[2 * m + 1] == 0.0) {   // kind 0, as in the loop of the static discs
        k2 = 1.0; w = s.wobs;
        const double arg = r * r - (dx * dx + dy * dy);
        e = exp(fmin(arg, 6.907755278982137));
        f = arg > 6.907755278982137 ? 1e3 * (1.0 + arg - 6.907755278982137) : e;
        cost_ref += w * e;
      } else {                        // kind 1
        k2 = (FIT_OBS_K / r) * (FIT_OBS_K / r);
        e = exp(-(dx * dx + dy * dy) * k2);
        cost_ref += s.wobs * e;
        w = s.wobs / k2;
        f = e;
      }
      const double we = w * e;
      obj += w * f;
      if (gx) {
        *gx += -k2 * we * dx; *gy += -k2 * we * dy;
        *dxx += k2 * k2 * we * dx * dx; *dxy += k2 * k2 * we * dx * dy; *dyy += k2 * k2 * we * dy * dy;
      }
    }
  }
  if constexpr (PAIRS) {
    if (s.wcol > 0.0) {                         // CostCollision against every frozen partner of the set
#pragma clang loop unroll(disable)
      for (unsigned m = pmask; m != 0u; m &= m - 1u) {
        const double *__restrict__ pj = partner + (size_t)__builtin_ctz(m) * NLP_NV * pstride;     // aircraft j's x plane; y follows
        const double dx = x - pj[pidx], dy = y - pj[pidx + pstride];
        const double e = exp(-(dx * dx + dy * dy) * s.kc2);
        cost_ref += s.wcol * e;
        const double we = s.wcol / s.kc2 * e;
        obj += we;
        if (gx) {
          *gx += -s.kc2 * we * dx; *gy += -s.kc2 * we * dy;
          *dxx += s.kc2 * s.kc2 * we * dx * dx; *dxy += s.kc2 * s.kc2 * we * dx * dy; *dyy += s.kc2 * s.kc2 * we * dy * dy;
        }
      }
    }
  } else if (partner != nullptr && s.wcol > 0.0) {     // CostCollision against the frozen partner (src/d2d/multiopty_utils.py:120-153)
    const double dx = x - partner[pidx], dy = y - partner[pidx + pstride];
    const double e = exp(-(dx * dx + dy * dy) * s.kc2);
    cost_ref += s.wcol * e;
    const double we = s.wcol / s.kc2 * e;
    obj += we;
    if (gx) {
      *gx += -s.kc2 * we * dx; *gy += -s.kc2 * we * dy;
      *dxx += s.kc2 * s.kc2 * we * dx * dx; *dxy += s.kc2 * s.kc2 * we * dx * dy; *dyy += s.kc2 * s.kc2 * we * dy * dy;
    }
  }
}

// ---- per-problem workspace (WS_TOTAL * N doubles) ---------------------------------------------------------------------------
// Data that the node-parallel phases touch lives in planes of N doubles ([component][node]: lane = node reads 64 consecutive
// doubles).  What the two serial recursions read and write is NODE-major ([node][component]): one base address per node and
// immediate offsets (plane-major, every component would need its own 64-bit address -- measured: that address arithmetic
// alone cost more than the block arithmetic).
enum {
  WS_ZL = 0, WS_ZU = 5,                  // bound duals (5 + 5 planes)
  WS_MU = 10,                            // scaled multiplier estimates (3 planes) unless the caller wants them (mult)
  WS_DW = 13,                            // step (5 planes)
  WS_RHS = 18,                           // right-hand side (5 planes)
  WS_EL = 23,                            // local elimination of (phi, v) (17 planes): 1/l00, l10, 1/l11; Qt [j][k] (6); Rt [j][k] (6); tt (2)
  WS_UP = 40,                            // what node i hands to node i-1 (9 planes): Rt^T Rt lower triangle (6), Rt^T tt (3)
  WS_SIN = 49,                           // reduced node [N][18]: D' lower triangle (6), E' [a][k] (9), t' (3)
  WS_SF = 67,                            // factor of the reduced system [N][18]: L (6, RECIPROCAL diagonal), Lo [a][k] (9), y (3)
  WS_DS = 85,                            // reduced step [N][3]
  WS_TOTAL = 88,
  EL_LP = 0, EL_Q = 3, EL_R = 9, EL_T = 15,
  UP_RR = 0, UP_RT = 6,
  SIN_D = 0, SIN_E = 6, SIN_T = 15, SIN_N = 18,
  SF_L = 0, SF_LO = 6, SF_Y = 15, SF_N = 18
};
// FREE instantiations (d2d_nlp_solve_free) keep the planes above and add, behind them, what the border column b of the Newton system
// needs: b itself, its (phi, v) part after the local elimination, the solution y = A^-1 b, and a second set of reduced-node records
// and reduced steps for the second pass of the cyclic reduction (which overwrites its records).
enum {
  WSF_B = WS_TOTAL,                      // border column b (5 planes)
  WSF_TB = WSF_B + 5,                    // LP^-1 b_pv (2 planes): the twin of EL_T
  WSF_Y = WSF_TB + 2,                    // y = A^-1 b (5 planes)
  WSF_SIN2 = WSF_Y + 5,                  // reduced node [N][18] with b's reduced right-hand side in the place of t'
  WSF_DS2 = WSF_SIN2 + SIN_N,            // reduced y [N][3]
  WSF_TOTAL = WSF_DS2 + 3
};

struct NlpProb {
  int N;
  double h;
  double *W;                 // [5][N] node values
  double *ws;                // WS_TOTAL * N doubles (see above)
  double *mu;                // [3][N]
  const double *partner;     // [2][N] or null; PAIRS instantiations: the scenario's W [n_ac][5][N]
  unsigned pmask;            // PAIRS instantiations: the partner set (bit j = aircraft j of the scenario), wave-uniform; else 0
  double *lds;               // this wavefront's NLP_LDS_DOUBLES doubles of LDS (nlp_assemble: neighbour hand-over, record transposition)
  const d2d_wind_field *wf;  // WIND instantiations (d2d_nlp_solve_wind): the field of the equalities, node i at t0 + i h; else null
  double t0;
};
// MOV instantiations: the problem with its moving discs (the others keep NlpProb as it is)
struct NlpMovProb : NlpProb {
  NlpMovSet mv;
};
// VIA instantiations (d2d_nlp_solve_via, d2d_nlp_solve_groups_via): the problem with the fixed set of its nodes.  vm [N], bits 0..2 of
// vm[i] = x, y, psi of node i are fixed variables: 7 at both ends (the end conditions), the pins of the via table in between.  The
// start pass of nlp_solve_one writes the plane; every pass that asks nlp_fixed elsewhere reads vm[i] with the node's values.
struct NlpViaProb : NlpMovProb {
  const int32_t *vm;
};
// FREE instantiations (d2d_nlp_solve_free): the problem with its free time step.  The solver's unknown is u = 1 / h, in which every
// equality is linear; h above is kept equal to 1 / u.  Wave-uniform values: u in (ulo, uhi) = (1 / h_hi, 1 / h_lo), its two bound
// duals, and kd = k_dur (N - 1), the weight of the duration term kd / u of the objective.
struct NlpFreeProb : NlpProb {
  double u, ulo, uhi, zul, zuu, kd;
};
// what nlp_assemble hands back for the row of u: rho sum (c + mu) . dc/du and rho sum |dc/du|^2 over the equalities
struct NlpFreeRow {
  double gu, dd;
};
// KEEP instantiations (d2d_nlp_solve_keepout): the problem with its hard keep-out discs.  discs [n][3] = (cx, cy, R), wave-uniform, a row
// with R <= 0 absent; z [n][N] the duals of  g_im = |p_i - c_m|^2 - R_m^2 > 0  (disc m's plane: z[m * N + i], lane = node), 0 at the two end
// nodes and for absent discs.  Every pass walks the discs in a ROLLED loop, ascending m, like the moving discs of nlp_exp_terms.
struct NlpKeepSet {
  const double *discs;
  double *z;
  int n;
};
struct NlpKeepProb : NlpProb {
  NlpKeepSet keep;
};
// KMOV instantiations (d2d_nlp_solve_keepout_moving, d2d_nlp_solve_groups_keepout): hard discs that MOVE.  discs is the table disc [n][2]
// of d2d_moving_obstacles, (R, kind) with R the node radius and R <= 0 absent (the kind is checked with the track and not read), and
// ctr the centre planes [n][2][N] that nlp_mov_sample_kernel wrote ahead of the solve: disc m's centre at node i is ctr[(2 m) * N + i],
// ctr[(2 m + 1) * N + i], lane = node.  The centres are data: every pass is the static one with the node's own centre, both planes
// requested BEFORE the branch on R > 0 (absent slots hold valid planes; a load inside the branch is a memory wait of its own).
struct NlpKeepMovSet : NlpKeepSet {
  const double *ctr;
};
struct NlpKeepMovProb : NlpProb {
  NlpKeepMovSet keep;
};
// KMOV: the discs' sums of two products, with the contraction the STATIC kernels have pinned by hand: ax bx + ay by as fma(ax, bx, ay by)
// and g as fma(-R, R, .).  Left to the compiler, the instantiations with centres in vector registers fuse the other product (seen in
// the ISA: dy dy + dx dx for the static kernels' dx dx + dy dy), an ulp per step that a full solve amplifies -- and tracks that stand
// still are to give d2d_nlp_solve_keepout's bytes.  The static instantiations keep their expressions: their code does not change.
__device__ __forceinline__ double nlp_dot2(double ax, double bx, double ay, double by) { return fma(ax, bx, ay * by); }
__device__ __forceinline__ double nlp_keep_g(double dx, double dy, double R) { return fma(-R, R, nlp_dot2(dx, dx, dy, dy)); }
// FENCE instantiations (d2d_nlp_solve_fence, d2d_nlp_solve_groups_fence): the problem INSIDE a convex polygon, a set of half-planes.
// edges [n][4] = (ax, ay, b, kap), wave-uniform, |a| = 1 the outward normal, a row with ax = ay = 0 absent; z [n][N] the duals of
// g_ik = b_k - (ax_k x_i + ay_k y_i) > 0  (edge k's plane: z[k * N + i], lane = node), 0 at the two end nodes and for absent edges.  The
// constraint is linear: grad g = -a, no curvature of its own, and the ratio test is exact.  Every pass walks the edges in a ROLLED loop,
// ascending k, after the discs; a . p is fma(ax, x, ay y) everywhere (nlp_fence_g, nlp_dot2), so that every instantiation -- and a later
// one that holds the edges in other registers -- rounds alike (the KMOV note below says why that is not left to the compiler).
struct NlpFenceSet {
  const double *edges;
  double *z;
  int n;
};
// (the static hard discs ride along: KEEP && FENCE reads both sets; FENCE alone, the group kernel, leaves keep unread)
struct NlpFenceProb : NlpKeepProb {
  NlpFenceSet fence;
};
// (how both sets travel in NlpExtra: through its keep pointer, as NlpKeepMovSet does -- the aggregate keeps its size, and with it the
// code of every instantiation that was there before)
struct NlpKeepFenceSet : NlpKeepSet {
  NlpFenceSet fence;
};
// FREE with KEEP and FENCE (d2d_nlp_solve_free_fence): both sets and the free step (the members of NlpFreeProb, under the same names)
struct NlpFreeFenceProb : NlpFenceProb {
  double u, ulo, uhi, zul, zuu, kd;
};
__device__ __forceinline__ bool nlp_fence_present(const double *__restrict__ e) { return e[0] != 0.0 || e[1] != 0.0; }
__device__ __forceinline__ double nlp_fence_g(const double *__restrict__ e, double x, double y) { return e[2] - nlp_dot2(e[0], x, e[1], y); }
template <unsigned F, typename X = NlpFeatures<F>>
using NlpProbT = std::conditional_t<X::FREE && (X::KEEP || X::FENCE), NlpFreeFenceProb, std::conditional_t<X::FENCE, NlpFenceProb, std::conditional_t<X::KEEP, std::conditional_t<X::KMOV, NlpKeepMovProb, NlpKeepProb>,
                                    std::conditional_t<X::FREE, NlpFreeProb, std::conditional_t<X::VIA, NlpViaProb, std::conditional_t<X::MOV, NlpMovProb, NlpProb>>>>>>;
template <unsigned F> using NlpProbV = NlpProbT<F & ~(NLP_MOV | NLP_FREE)>;       // for the passes that read no soft disc and no u
template <unsigned F, typename X = NlpFeatures<F>>             // the set type that NlpExtra's keep pointer stands for
using NlpKeepSetT = std::conditional_t<X::FENCE, NlpKeepFenceSet, std::conditional_t<X::KMOV, NlpKeepMovSet, NlpKeepSet>>;
template <unsigned F, typename PB> __device__ __forceinline__ const NlpMovSet *nlp_mov_set(const PB &pb) {
  if constexpr (NlpFeatures<F>::MOV) return &pb.mv;
  else return nullptr;
}
// Objective model of d2d_nlp_solve_model (user cost plug-ins, opty/direct_collocation.py): this problem's planes.  The objective of
// that instantiation is  m(W) = sum_i g_i.d_i + 1/2 d_i^T H_i d_i,  d_i = W_i - Wc_i, on top of the structured terms (which the
// host's row zeroes); H_i is held as its upper triangle, row by row (nlp_hidx).
struct NlpModel {
  const double *g;           // [5][N]
  const double *H;           // [15][N]
  const double *Wc;          // [5][N]
};
__host__ __device__ constexpr int nlp_hidx(int a, int c) { return a * NLP_NV - a * (a - 1) / 2 + (c - a); }     // a <= c
// LDS of one wavefront: up [65][9] (what a node hands to the node before it; row 64 = the first node of the chunk processed before),
// then rec [64][19] (the reduced-node records of a chunk, odd stride: conflict-free both ways)
#define NLP_LDS_UP 0
#define NLP_LDS_REC (65 * 9)
#define NLP_REC_STRIDE 19
#define NLP_BCR_STRIDE 19                 // odd: a lane per node reads its record without 8-way bank conflicts
#define NLP_BCR_LDS_NODES 121
#define NLP_LDS_DOUBLES 2304              // >= 65 * 9 + 64 * NLP_REC_STRIDE (assembly) and >= NLP_BCR_LDS_NODES * NLP_BCR_STRIDE (cyclic reduction)
static_assert(64 * NLP_BCR_STRIDE >= 65 * 9 && NLP_REC_STRIDE == NLP_BCR_STRIDE, "nlp_assemble rec_lds: records of the chunks above the first lie behind the hand-over rows");
#define NLP_T(i) (pb.t0 + (double)(i) * pb.h)       // (one multiply-add: not accumulated from node to node)
#define NLP_W(c, i) pb.W[(c) * pb.N + (i)]
#define NLP_P(plane, i) pb.ws[(plane) * pb.N + (i)]
#define NLP_MU(k, i) pb.mu[(k) * pb.N + (i)]
#define NLP_DW(c, i) NLP_P(WS_DW + (c), i)
#define NLP_RHS(c, i) NLP_P(WS_RHS + (c), i)
#define NLP_EL(k, i) NLP_P(WS_EL + (k), i)
#define NLP_UP(k, i) NLP_P(WS_UP + (k), i)
#define NLP_SIN(k, i) pb.ws[(size_t)WS_SIN * pb.N + (i) * SIN_N + (k)]
#define NLP_SF(k, i) pb.ws[(size_t)WS_SF * pb.N + (i) * SF_N + (k)]
#define NLP_DS(k, i) pb.ws[(size_t)WS_DS * pb.N + (i) * 3 + (k)]

// stores of one phase -> loads of the next phase by OTHER lanes of the same wavefront (one wavefront owns a problem)
__device__ __forceinline__ void nlp_phase_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wave_min(double v) { return -wave_max(-v); }

__device__ __forceinline__ double nlp_first_lane(double v) {              // the value lane 0 holds, in every lane
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// collocation residual of node i (>= 1) from the states of node i-1 and the node itself (oracle/nlp.py constraints).
// WIND: the wind of the equalities is + the field wf at the node's own time t and position (tests/nlp_wind_ref.py constraints)
template <bool WIND = false>
__device__ __forceinline__ void nlp_constraint(const NlpScen &s, double h, const double wp[3], const double w[NLP_NV], double c[3],
                                               const d2d_wind_field *wf = nullptr, double t = 0.0) {
  double sp, cp;
  sincos(w[2], &sp, &cp);
  if constexpr (WIND) {
    const WindVec wv = wind_at(*wf, t, w[0], w[1]);
    c[0] = (w[0] - wp[0]) / h - w[4] * cp + wv.x;
    c[1] = (w[1] - wp[1]) / h - w[4] * sp + wv.y;
  } else {
    c[0] = (w[0] - wp[0]) / h - w[4] * cp + s.wx;
    c[1] = (w[1] - wp[1]) / h - w[4] * sp + s.wy;
  }
  c[2] = (w[2] - wp[2]) / h - FIT_G / w[4] * tan(w[3]);
}

__device__ __forceinline__ bool nlp_fixed(int i, int N, int c) { return c < 3 && (i == 0 || i == N - 1); }
// VIA: the node's mask m = vm[i] answers instead (nlp_via_mask: 0 in the other instantiations, where it is not read)
template <unsigned F>
__device__ __forceinline__ bool nlp_fixed_at(int i, int N, int c, int m) {
  if constexpr (NlpFeatures<F>::VIA) return c < 3 && ((m >> c) & 1) != 0;
  else return nlp_fixed(i, N, c);
}
template <unsigned F, typename PB>
__device__ __forceinline__ int nlp_via_mask(const PB &pb, int i) {
  if constexpr (NlpFeatures<F>::VIA) return pb.vm[i];
  else return 0;
}

// Merit function of the inner problem at W + a*dw: objective + rho sum (c + mu)^2 - mub sum log(slacks); +inf outside the box.
// Node-parallel (lane = node, chunks of 64) + wave reductions.  All results are wave-uniform.
// FREE: ut is the trial value of u = 1 / h (u + a du): the equalities are read at 1 / ut, and the duration term kd / ut, the barrier of
// u's box and the value +inf outside it join the sums (cost_ref_out: the reference's cost() + k_dur (N - 1) h).
// KEEP: - mub log g of every (interior node, disc) joins the barrier (one more log per node, of the product), +inf when a g <= 0.
// FENCE: - mub log g of every (interior node, edge) likewise, a log of its own behind the discs'.
template <unsigned F>
__device__ double nlp_merit(const NlpProbT<F> &pb, const NlpScen &s, const double *__restrict__ sc, int lane, double a, double rho,
                            double mub, double *cost_ref_out, double *feas_out, const NlpModel &md, [[maybe_unused]] double ut = 0.0) {
  NLP_FEATURES(F);
  const int N = pb.N;
  [[maybe_unused]] const double ht = FREE ? 1.0 / ut : 0.0;
  double val = 0.0, bar = 0.0, cref = 0.0, feas = 0.0, phi2max = 0.0;
  int outside = 0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i < N) {
      // (every value the node needs is requested up front, from clamped indices where a neighbour does not exist: a load inside a
      // branch is a memory round trip of its own -- the compiler does not speculate loads -- and a Newton step had forty of those)
      const int im = i >= 1 ? i - 1 : 0;
      double w[NLP_NV], wp[3], dwl[NLP_NV], dwp[3], muv[3];
#pragma unroll
      for (int c = 0; c < NLP_NV; ++c) { w[c] = NLP_W(c, i); dwl[c] = NLP_DW(c, i); }
#pragma unroll
      for (int c = 0; c < 3; ++c) { wp[c] = NLP_W(c, im); dwp[c] = NLP_DW(c, im); muv[c] = NLP_MU(c, i); }
      [[maybe_unused]] const int vmi = nlp_via_mask<F>(pb, i);
      if (a != 0.0) {
#pragma unroll
        for (int c = 0; c < NLP_NV; ++c) w[c] += a * dwl[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) wp[c] += a * dwp[c];
      }
      if (i < 1) { wp[0] = 0.0; wp[1] = 0.0; wp[2] = 0.0; }
      double prod = 1.0;
#pragma unroll
      for (int c = 0; c < NLP_NV; ++c) {
        if (nlp_fixed_at<F>(i, N, c, vmi)) continue;
        if (s.lo[c] > -1e299) { const double sl = w[c] - s.lo[c]; if (!(sl > 0.0)) outside = 1; prod *= (sl > 0.0 ? sl : 1.0); }
        if (s.hi[c] < 1e299) { const double su = s.hi[c] - w[c]; if (!(su > 0.0)) outside = 1; prod *= (su > 0.0 ? su : 1.0); }
      }
      bar += log(prod);               // one log per node: at most ten slacks in [1e-12, 1e3], their product stays in range
      if constexpr (KEEP) {
        if (i >= 1 && i < N - 1) {
          const double *__restrict__ dk = pb.keep.discs;
          double pk = 1.0;            // at most D2D_MAX_KEEP values g in [1e-12, 1e8]: in range too
#pragma clang loop unroll(disable)
          for (int m = 0; m < pb.keep.n; ++m) {
            [[maybe_unused]] double cxm = 0.0, cym = 0.0;
            if constexpr (KMOV) { cxm = pb.keep.ctr[(size_t)(2 * m) * N + i]; cym = pb.keep.ctr[(size_t)(2 * m + 1) * N + i]; }
            const double R = dk[KMOV ? 2 * m : 3 * m + 2];
            if (!(R > 0.0)) continue;
            const double dx = w[0] - (KMOV ? cxm : dk[3 * m]), dy = w[1] - (KMOV ? cym : dk[3 * m + 1]);
            const double gk = KMOV ? nlp_keep_g(dx, dy, R) : dx * dx + dy * dy - R * R;
            if (!(gk > 0.0)) outside = 1;
            pk *= (gk > 0.0 ? gk : 1.0);
          }
          bar += log(pk);
        }
      }
      if constexpr (FENCE) {
        if (i >= 1 && i < N - 1) {
          double pf = 1.0;            // at most D2D_MAX_FENCE values g in [1e-12, 1e4]: in range too
#pragma clang loop unroll(disable)
          for (int k = 0; k < pb.fence.n; ++k) {
            const double *__restrict__ e = pb.fence.edges + 4 * k;
            if (!nlp_fence_present(e)) continue;
            const double gk = nlp_fence_g(e, w[0], w[1]);
            if (!(gk > 0.0)) outside = 1;
            pf *= (gk > 0.0 ? gk : 1.0);
          }
          bar += log(pf);
        }
      }
      const double dv = w[4] - s.vsp;
      double obj = s.skv * dv * dv + s.skphi * w[3] * w[3];
      if constexpr (MODEL) {          // g.d + 1/2 d^T H d
        double d[NLP_NV];
#pragma unroll
        for (int c = 0; c < NLP_NV; ++c) d[c] = w[c] - md.Wc[c * N + i];
#pragma unroll
        for (int r = 0; r < NLP_NV; ++r) {
          double t = md.g[r * N + i] + 0.5 * md.H[nlp_hidx(r, r) * N + i] * d[r];
#pragma unroll
          for (int c = r + 1; c < NLP_NV; ++c) t += md.H[nlp_hidx(r, c) * N + i] * d[c];
          obj += d[r] * t;
        }
      }
      phi2max = fmax(phi2max, w[3] * w[3]);
      cref += obj;
      nlp_exp_terms<F>(s, sc, pb.partner, i, N, w[0], w[1], obj, cref, pb.pmask, nlp_mov_set<F>(pb));
      val += obj;
      if (i >= 1) {
        double c3[3];
        if constexpr (FREE) nlp_constraint(s, ht, wp, w, c3);
        else
        nlp_constraint<WIND>(s, pb.h, wp, w, c3, pb.wf, NLP_T(i));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double cm = c3[k] + muv[k];
          val += rho * cm * cm;
          feas = fmax(feas, fabs(c3[k]));
        }
      }
    }
  }
  val = wave_sum(val); bar = wave_sum(bar);
  cref = wave_sum(cref);
  if (s.sbank > 0.0) {                       // CostBank max mode (src/d2d/opty_utils.py:68-82): obj_scale * kbank * max_i phi_i^2
    const double bk = s.sbank * wave_max(phi2max);
    val += bk; cref += bk;
  }
  if constexpr (FREE) {
    const double dur = pb.kd / ut, sl = ut - pb.ulo, su = pb.uhi - ut;
    val += dur; cref += dur;
    if (!(sl > 0.0) || !(su > 0.0)) outside = 1;
    else bar += log(sl * su);
  }
  if (cost_ref_out) *cost_ref_out = cref;
  if (feas_out) *feas_out = wave_max(feas);
  const bool any_out = __builtin_amdgcn_ballot_w64(outside != 0) != 0ull;
  if (any_out || !(fabs(val) <= 1.79e308)) return INFINITY;
  return val - mub * bar;
}

// 1/sqrt(v), v > 0 (normal range): hardware estimate + two Newton steps (the pivots of the serial recursion are a dependent
// chain -- the library's sqrt followed by a division is four times as long)
__device__ __forceinline__ double nlp_rsqrt(double v) {
  double y = __builtin_amdgcn_rsq(v);
  const double hv = 0.5 * v;
  y = fma(y, fma(-hv * y, y, 0.5), y);
  y = fma(y, fma(-hv * y, y, 0.5), y);
  return y;
}

// Assembly + local elimination (node-parallel, one pass, the 5x5 blocks never leave the registers): half gradient g, half Hessian
// blocks D (diagonal) and E (i, i-1) of the barrier-AL Lagrangian incl. the constraint curvature, barrier diagonal, damping,
// right-hand side; then the elimination of (phi, v) described below.  Returns the barrier KKT error of the inner problem
// (wave-uniform; it does not depend on the damping); *pd_out = false if a 2x2 pivot is not positive.
// node with the largest |phi| at the current iterate (first on ties), wave-uniform
__device__ int nlp_bank_argmax(const NlpProb &pb, int lane) {
  const int N = pb.N;
  double best = -1.0;
  int istar = 0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    const double a = i < N ? fabs(NLP_W(3, i)) : -1.0;
    const double m = wave_max(a);
    if (m > best) { best = m; istar = i0 + (int)__builtin_ctzll(__ballot(a == m)); }
  }
  return __builtin_amdgcn_readfirstlane(istar);
}

// imax (CostBank max mode, s.sbank > 0): the node whose bank angle is the largest at the current iterate -- the reference's
// cost_grad is one-hot there (2 obj_scale kbank phi_imax), the step's model carries the term sbank * phi_imax^2 on that node
// alone (the maximiser frozen for the step; the merit function of the line search is the true max)
// WIND (d2d_nlp_solve_wind): the constraint that ends at node i reads the field at (t_i, x_i, y_i): with J = d(wx, wy)/d(x, y) there,
// Ac gains J on its (x, y) columns and D the constraint curvature rho (c + mu)_0 Hess(wx) + rho (c + mu)_1 Hess(wy) on its (x, y)
// block; node i+1's constraint sees node i through -1/h only, so the has_next terms and the structure of E do not change.
// VIA: the rows and columns of a pinned component are the identity with right-hand side 0, as at the ends, and the columns of E_i that
// belong to pinned components of node i-1 are zero (at the ends: all of E_1) -- before the elimination, so Rt carries none of them.
// FREE: the border column b of the Newton system, bordered by the row of u = 1 / h (c = (s_i - s_{i-1}) u - f(s_i): dc/du = the node
// difference dl, cross curvature +1 on the node's own (x, y, psi) and -1 on its predecessor's):
//   b_i = rho Ac^T dl_i + rho (c + mu)_i  on node i  [own equality]   - rho u dl_{i+1} - rho (c + mu)_{i+1}  on (x, y, psi)_i  [next one]
// b goes through the same elimination of (phi, v) as the right-hand side (ttb, its hand-over, its reduced part, which lands in the
// t' slots of a second set of records for the second pass of the cyclic reduction); fr_out: the sums of the row of u.  rec_lds is
// false for this instantiation: both passes load their records from the workspace.
// KEEP: disc m at an interior node i, d = p_i - c_m, g = |d|^2 - R^2, dual z: the stationarity rows of (x, y) gain - z 2d, the right-hand
// side + (mub / g) 2d, the (x, y) corner of D (half convention)  2 (z / g) d d^T - z I  -- the - z I is the constraint's own, negative,
// curvature: a corner that it makes indefinite fails a pivot of the reduced system and the caller raises the damping -- and the KKT
// error |z g - mub|.  Nothing else of the pass changes.
// FENCE: edge k at an interior node i, g = b - a . p, grad g = -a, dual z: the stationarity rows of (x, y) gain + z a, the right-hand side
// - (mub / g) a, the (x, y) corner of D (half convention)  1/2 (z / g) a a^T  -- positive semidefinite, the constraint has no curvature --
// and the KKT error |z g - mub|.  The sums kst, krh are the discs' (of grad g), so both families leave through the same two lines below.
template <unsigned F>
__device__ double nlp_assemble(const NlpProbT<F> &pb, const NlpScen &s, const double *__restrict__ sc, int lane, double rho, double mub,
                               double lam, bool *pd_out, int imax, bool rec_lds, const NlpModel &md, [[maybe_unused]] NlpFreeRow *fr_out = nullptr) {
  NLP_FEATURES(F);
  const int N = pb.N;
  const double h = pb.h, ih = 1.0 / h;
  double err = 0.0;
  int bad = 0;
  constexpr int UPN = FREE ? 12 : 9;          // doubles a node hands to the node before it (FREE: + Rt^T ttb)
  [[maybe_unused]] double gu = 0.0, dd = 0.0;
  // The chunks of 64 nodes are visited from the LAST to the first: node i needs what node i+1 hands to it (the hand-over of the
  // elimination, below), and for the last lane of a chunk that is the first node of the chunk visited before.
  double *lds_up = pb.lds + NLP_LDS_UP, *lds_rec = pb.lds + (FREE ? 65 * UPN : NLP_LDS_REC);
  [[maybe_unused]] double wnx_first = 0.0, wny_first = 0.0;      // WIND: the field at the first node of the chunk visited before (lane 63's next node)
  for (int i0 = ((N - 1) / 64) * 64; i0 >= 0; i0 -= 64) {
    const int i = i0 + lane;
    const bool live = i < N;
    double sinv[SIN_N], upv[UPN];
    [[maybe_unused]] double tbv[3] = {0.0, 0.0, 0.0};      // FREE: b's reduced right-hand side
    [[maybe_unused]] WindJet wj;                     // WIND: the field at this lane's node
    if (live) {
    const bool has_next = i + 1 < N;
    double rhsv[NLP_NV];
    [[maybe_unused]] double bv[NLP_NV] = {0, 0, 0, 0, 0};
    double wp[3] = {0, 0, 0}, wc[NLP_NV], wn[NLP_NV] = {0, 0, 0, 0, 1};
    double cc[3] = {0, 0, 0}, cn[3] = {0, 0, 0};     // (c + mu) of the constraint that ends at this node / at the next one
    // (all loads of the node up front, neighbours from clamped indices: see nlp_merit)
    const int im = i >= 1 ? i - 1 : 0, ip = has_next ? i + 1 : i;
    double zlv[NLP_NV], zuv[NLP_NV], mu_c[3], mu_n[3];
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) { wc[c] = NLP_W(c, i); wn[c] = NLP_W(c, ip); zlv[c] = NLP_P(WS_ZL + c, i); zuv[c] = NLP_P(WS_ZU + c, i); }
#pragma unroll
    for (int c = 0; c < 3; ++c) { wp[c] = NLP_W(c, im); mu_c[c] = NLP_MU(c, i); mu_n[c] = NLP_MU(c, ip); }
    [[maybe_unused]] const int vmi = nlp_via_mask<F>(pb, i), vmp = nlp_via_mask<F>(pb, im);
    if (i < 1) { wp[0] = 0.0; wp[1] = 0.0; wp[2] = 0.0; }
    // WIND: the field at this node -- value, Jacobian, second derivatives in one pass -- for every live lane; the value at the
    // NEXT node, which cn needs, comes from the neighbouring lane (NLP_WIND_NEXT_SHUFFLE, the default) or from a second, value-only
    // evaluation: DESIGN.md 5.10 has the A/B
    [[maybe_unused]] double wnx = 0.0, wny = 0.0;
    if constexpr (WIND) {
      wj = wind_eval2(*pb.wf, NLP_T(i), wc[0], wc[1]);
#if NLP_WIND_NEXT_SHUFFLE
      wnx = __shfl_down(wj.w[0], 1); wny = __shfl_down(wj.w[1], 1);
      if (lane == 63) { wnx = wnx_first; wny = wny_first; }
#endif
    }
    if (has_next) {
      if constexpr (WIND) {
#if NLP_WIND_NEXT_SHUFFLE
        double spn, cpn;
        sincos(wn[2], &spn, &cpn);
        cn[0] = (wn[0] - wc[0]) / h - wn[4] * cpn + wnx;
        cn[1] = (wn[1] - wc[1]) / h - wn[4] * spn + wny;
        cn[2] = (wn[2] - wc[2]) / h - FIT_G / wn[4] * tan(wn[3]);
#else
        nlp_constraint<true>(s, h, wc, wn, cn, pb.wf, NLP_T(i + 1));
#endif
      } else {
        nlp_constraint(s, h, wc, wn, cn);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) cn[k] += mu_n[k];
    } else {
      wn[0] = 0.0; wn[1] = 0.0; wn[2] = 0.0; wn[3] = 0.0; wn[4] = 1.0;
    }
    double g[NLP_NV] = {0, 0, 0, 0, 0};
    [[maybe_unused]] double kst[2] = {0.0, 0.0}, krh[2] = {0.0, 0.0};      // KEEP: sum z 2d and sum (mub / g) 2d over the discs
    double D[NLP_NV][NLP_NV];
#pragma unroll
    for (int a = 0; a < NLP_NV; ++a)
#pragma unroll
      for (int c = 0; c < NLP_NV; ++c) D[a][c] = 0.0;
    D[4][4] += s.skv; g[4] += s.skv * (wc[4] - s.vsp);
    D[3][3] += s.skphi; g[3] += s.skphi * wc[3];
    if (i == imax) { D[3][3] += s.sbank; g[3] += s.sbank * wc[3]; }
    if constexpr (MODEL) {            // half gradient 1/2 (g + H d), half Hessian 1/2 H (H loaded here, not with the node's other values)
      double d[NLP_NV];
#pragma unroll
      for (int c = 0; c < NLP_NV; ++c) { d[c] = wc[c] - md.Wc[c * N + i]; g[c] += 0.5 * md.g[c * N + i]; }
#pragma unroll
      for (int r = 0; r < NLP_NV; ++r) {
#pragma unroll
        for (int c = r; c < NLP_NV; ++c) {
          const double hv = 0.5 * md.H[nlp_hidx(r, c) * N + i];
          D[r][c] += hv; g[r] += hv * d[c];
          if (c != r) { D[c][r] += hv; g[c] += hv * d[r]; }
        }
      }
    }
    {
      double obj = 0.0, cref = 0.0;
      nlp_exp_terms<F>(s, sc, pb.partner, i, N, wc[0], wc[1], obj, cref, pb.pmask, nlp_mov_set<F>(pb), &g[0], &g[1], &D[0][0], &D[0][1], &D[1][1]);
      if constexpr (KEEP) {
        if (i >= 1 && i < N - 1) {
          const double *__restrict__ dk = pb.keep.discs;
#pragma clang loop unroll(disable)
          for (int m = 0; m < pb.keep.n; ++m) {
            [[maybe_unused]] double cxm = 0.0, cym = 0.0;
            if constexpr (KMOV) { cxm = pb.keep.ctr[(size_t)(2 * m) * N + i]; cym = pb.keep.ctr[(size_t)(2 * m + 1) * N + i]; }
            const double R = dk[KMOV ? 2 * m : 3 * m + 2];
            if (!(R > 0.0)) continue;
            const double dx = wc[0] - (KMOV ? cxm : dk[3 * m]), dy = wc[1] - (KMOV ? cym : dk[3 * m + 1]);
            const double gk = KMOV ? nlp_keep_g(dx, dy, R) : dx * dx + dy * dy - R * R, z = pb.keep.z[(size_t)m * N + i], ig = 1.0 / gk, zg = z * ig, mg = mub * ig;
            kst[0] += 2.0 * z * dx; kst[1] += 2.0 * z * dy;
            krh[0] += 2.0 * mg * dx; krh[1] += 2.0 * mg * dy;
            D[0][0] += 2.0 * zg * dx * dx - z; D[0][1] += 2.0 * zg * dx * dy; D[1][1] += 2.0 * zg * dy * dy - z;
            err = fmax(err, fabs(z * gk - mub));
          }
        }
      }
      if constexpr (FENCE) {
        if (i >= 1 && i < N - 1) {
#pragma clang loop unroll(disable)
          for (int k = 0; k < pb.fence.n; ++k) {
            const double *__restrict__ e = pb.fence.edges + 4 * k;
            if (!nlp_fence_present(e)) continue;
            const double ax = e[0], ay = e[1], gk = nlp_fence_g(e, wc[0], wc[1]), z = pb.fence.z[(size_t)k * N + i], ig = 1.0 / gk, zg = 0.5 * (z * ig), mg = mub * ig;
            kst[0] = fma(-z, ax, kst[0]); kst[1] = fma(-z, ay, kst[1]);
            krh[0] = fma(-mg, ax, krh[0]); krh[1] = fma(-mg, ay, krh[1]);
            D[0][0] = fma(zg * ax, ax, D[0][0]); D[0][1] = fma(zg * ax, ay, D[0][1]); D[1][1] = fma(zg * ay, ay, D[1][1]);
            err = fmax(err, fabs(z * gk - mub));
          }
        }
      }
      D[1][0] = D[0][1];
    }
    double E[NLP_NV][3];                        // block (i, i-1): only the (x, y, psi) columns of node i-1 are non-zero
#pragma unroll
    for (int a = 0; a < NLP_NV; ++a) { E[a][0] = 0.0; E[a][1] = 0.0; E[a][2] = 0.0; }
    if (i >= 1) {
      double sp, cp;
      sincos(wc[2], &sp, &cp);
      const double tp = tan(wc[3]), vi = wc[4], sec2 = 1.0 + tp * tp;
      if constexpr (WIND) {
        cc[0] = (wc[0] - wp[0]) * ih - vi * cp + wj.w[0] + mu_c[0];
        cc[1] = (wc[1] - wp[1]) * ih - vi * sp + wj.w[1] + mu_c[1];
      } else {
        cc[0] = (wc[0] - wp[0]) * ih - vi * cp + s.wx + mu_c[0];
        cc[1] = (wc[1] - wp[1]) * ih - vi * sp + s.wy + mu_c[1];
      }
      cc[2] = (wc[2] - wp[2]) * ih - FIT_G / vi * tp + mu_c[2];
      double Ac[3][NLP_NV];                     // Jacobian of the constraint wrt this node
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < NLP_NV; ++c) Ac[k][c] = 0.0;
      Ac[0][0] = ih; Ac[0][2] = vi * sp; Ac[0][4] = -cp;
      Ac[1][1] = ih; Ac[1][2] = -vi * cp; Ac[1][4] = -sp;
      Ac[2][2] = ih; Ac[2][3] = -FIT_G * sec2 / vi; Ac[2][4] = FIT_G * tp / (vi * vi);
      if constexpr (WIND) { Ac[0][0] += wj.dx[0]; Ac[0][1] = wj.dy[0]; Ac[1][0] = wj.dx[1]; Ac[1][1] += wj.dy[1]; }
#pragma unroll
      for (int a = 0; a < NLP_NV; ++a) {
#pragma unroll
        for (int c = 0; c < NLP_NV; ++c) D[a][c] += rho * (Ac[0][a] * Ac[0][c] + Ac[1][a] * Ac[1][c] + Ac[2][a] * Ac[2][c]);
        g[a] += rho * (Ac[0][a] * cc[0] + Ac[1][a] * cc[1] + Ac[2][a] * cc[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) E[a][k] = -rho * Ac[k][a] * ih;
      }
      if constexpr (FREE) {
        const double dl[3] = {wc[0] - wp[0], wc[1] - wp[1], wc[2] - wp[2]};
#pragma unroll
        for (int a = 0; a < NLP_NV; ++a) bv[a] += rho * (Ac[0][a] * dl[0] + Ac[1][a] * dl[1] + Ac[2][a] * dl[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) { bv[k] += rho * cc[k]; gu += cc[k] * dl[k]; dd += dl[k] * dl[k]; }
      }
      // + rho (c + mu) Hessian(c): the constraint curvature of the Lagrangian
      const double m0 = rho * cc[0], m1 = rho * cc[1], m2 = rho * cc[2];
      D[2][2] += m0 * vi * cp + m1 * vi * sp;
      const double d24 = m0 * sp - m1 * cp;
      D[2][4] += d24; D[4][2] += d24;
      D[3][3] += -m2 * 2.0 * FIT_G * tp * sec2 / vi;
      const double d34 = m2 * FIT_G * sec2 / (vi * vi);
      D[3][4] += d34; D[4][3] += d34;
      D[4][4] += -m2 * 2.0 * FIT_G * tp / (vi * vi * vi);
      if constexpr (WIND) {
        D[0][0] += m0 * wj.xx[0] + m1 * wj.xx[1];
        const double d01 = m0 * wj.xy[0] + m1 * wj.xy[1];
        D[0][1] += d01; D[1][0] += d01;
        D[1][1] += m0 * wj.yy[0] + m1 * wj.yy[1];
      }
    }
    if (has_next) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { D[k][k] += rho * ih * ih; g[k] += -rho * cn[k] * ih; }
      if constexpr (FREE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) bv[k] += -rho * ih * (wn[k] - wc[k]) - rho * cn[k];
      }
    }
    // barrier terms, stationarity / complementarity error, right-hand side
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) {
      const bool fx = nlp_fixed_at<F>(i, N, c, vmi);
      double sig = 0.0, r = -2.0 * g[c], st = 2.0 * g[c];
      if (!fx && s.lo[c] > -1e299) {
        const double sl = wc[c] - s.lo[c], z = zlv[c], isl = 1.0 / sl;
        sig += z * isl; r += mub * isl; st -= z;
        err = fmax(err, fabs(z * sl - mub));
      }
      if (!fx && s.hi[c] < 1e299) {
        const double su = s.hi[c] - wc[c], z = zuv[c], isu = 1.0 / su;
        sig += z * isu; r -= mub * isu; st += z;
        err = fmax(err, fabs(z * su - mub));
      }
      if constexpr (KEEP || FENCE) {
        if (c < 2 && !fx) { r += krh[c]; st -= kst[c]; }
      }
      if (!fx) err = fmax(err, fabs(st));
      rhsv[c] = fx ? 0.0 : r;
      NLP_RHS(c, i) = rhsv[c];
      if constexpr (FREE) { if (fx) bv[c] = 0.0; NLP_P(WSF_B + c, i) = bv[c]; }
      D[c][c] += 0.5 * sig;
      if (!fx) D[c][c] += lam * fmax(fabs(D[c][c]), 1e-12);
      if (fx) {
#pragma unroll
        for (int a = 0; a < NLP_NV; ++a) { D[c][a] = 0.0; D[a][c] = 0.0; }
        D[c][c] = 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) E[c][k] = 0.0;
      }
    }
    if constexpr (VIA) {                        // columns of E that belong to the fixed variables of node i-1 (node 0: E is zero)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if ((vmp >> k) & 1) {
#pragma unroll
          for (int a = 0; a < NLP_NV; ++a) E[a][k] = 0.0;
        }
      }
    } else
    if (i == 1) {                               // columns of E that belong to the fixed variables of node 0
#pragma unroll
      for (int a = 0; a < NLP_NV; ++a) { E[a][0] = 0.0; E[a][1] = 0.0; E[a][2] = 0.0; }
    }
    // ---- elimination of (phi, v) of this node: P = LP LP^T, Qt = LP^-1 M[pv, s_i], Rt = LP^-1 M[pv, s_{i-1}], tt = LP^-1 rhs_pv / 2
    double P00 = D[3][3], v11;
    if (!(P00 > 0.0)) { bad = 1; P00 = 1.0; }
    const double i00 = nlp_rsqrt(P00), l10 = D[4][3] * i00;
    v11 = D[4][4] - l10 * l10;
    if (!(v11 > 0.0)) { bad = 1; v11 = 1.0; }
    const double i11 = nlp_rsqrt(v11);
    NLP_EL(EL_LP + 0, i) = i00; NLP_EL(EL_LP + 1, i) = l10; NLP_EL(EL_LP + 2, i) = i11;
    double Qt[2][3], Rt[2][3], tt[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Qt[0][k] = D[3][k] * i00; Qt[1][k] = (D[4][k] - l10 * Qt[0][k]) * i11;
      Rt[0][k] = E[3][k] * i00; Rt[1][k] = (E[4][k] - l10 * Rt[0][k]) * i11;
    }
    tt[0] = 0.5 * rhsv[3] * i00;
    tt[1] = (0.5 * rhsv[4] - l10 * tt[0]) * i11;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { NLP_EL(EL_Q + j * 3 + k, i) = Qt[j][k]; NLP_EL(EL_R + j * 3 + k, i) = Rt[j][k]; }
      NLP_EL(EL_T + j, i) = tt[j];
    }
    [[maybe_unused]] double ttb[2] = {0.0, 0.0};
    if constexpr (FREE) {                       // the border through the same elimination: ttb = LP^-1 b_pv
      ttb[0] = bv[3] * i00;
      ttb[1] = (bv[4] - l10 * ttb[0]) * i11;
      NLP_P(WSF_TB + 0, i) = ttb[0]; NLP_P(WSF_TB + 1, i) = ttb[1];
    }
    // what node i-1 gets from this node's elimination, and this node's own part of the reduced node
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int c = 0; c <= a; ++c) {
        upv[UP_RR + a * (a + 1) / 2 + c] = Rt[0][a] * Rt[0][c] + Rt[1][a] * Rt[1][c];
        sinv[SIN_D + a * (a + 1) / 2 + c] = D[a][c] - (Qt[0][a] * Qt[0][c] + Qt[1][a] * Qt[1][c]);
      }
      upv[UP_RT + a] = Rt[0][a] * tt[0] + Rt[1][a] * tt[1];
#pragma unroll
      for (int k = 0; k < 3; ++k) sinv[SIN_E + a * 3 + k] = E[a][k] - (Qt[0][a] * Rt[0][k] + Qt[1][a] * Rt[1][k]);
      sinv[SIN_T + a] = 0.5 * rhsv[a] - (Qt[0][a] * tt[0] + Qt[1][a] * tt[1]);
      if constexpr (FREE) {
        upv[9 + a] = Rt[0][a] * ttb[0] + Rt[1][a] * ttb[1];
        tbv[a] = bv[a] - (Qt[0][a] * ttb[0] + Qt[1][a] * ttb[1]);
      }
    }
    }
#if NLP_WIND_NEXT_SHUFFLE
    // (outside the live branch: every lane of the wave keeps the value, also the lanes beyond the end of the last chunk -- lane 63 of
    // the chunk below reads its own copy; lane 0 of a chunk is always live)
    if constexpr (WIND) { wnx_first = nlp_first_lane(wj.w[0]); wny_first = nlp_first_lane(wj.w[1]); }
#endif
    // ---- hand-over between neighbours, D'_i -= (Rt^T Rt)_{i+1}, t'_i -= (Rt^T tt)_{i+1}, through the LDS (the records used to make
    // a round trip through HBM for it), then the node-major records of the chunk transposed through the LDS so that they leave as
    // full 512-byte rows: 8-byte stores at a stride of 144 bytes reached the memory as partial sectors (WRITE_SIZE 1.6 x algorithmic)
    if (live) {
#pragma unroll
      for (int k = 0; k < UPN; ++k) lds_up[lane * UPN + k] = upv[k];
    }
    nlp_phase_sync();
    if (live && i + 1 < N) {
      const double *nb = lds_up + (lane + 1) * UPN;         // lane 63: row 64 = node i0 + 64, left there by the chunk visited before
#pragma unroll
      for (int k = 0; k < 6; ++k) sinv[SIN_D + k] -= nb[UP_RR + k];
#pragma unroll
      for (int a = 0; a < 3; ++a) sinv[SIN_T + a] -= nb[UP_RT + a];
      if constexpr (FREE) {
#pragma unroll
        for (int a = 0; a < 3; ++a) tbv[a] -= nb[9 + a];
      }
    }
    if constexpr (FREE) {
      if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) pb.ws[(size_t)WSF_SIN2 * N + (size_t)i * SIN_N + SIN_T + a] = tbv[a];
      }
    }
    if (rec_lds) {
      // The cyclic reduction that follows works in this wave's LDS block on records [node][NLP_BCR_STRIDE] (N <= NLP_BCR_LDS_NODES):
      // the records go there directly -- no store to the workspace, no load back (three memory round trips of a Newton step).
      // Chunks above the first lie behind the hand-over rows (64 * 19 >= 65 * 9); the first chunk's own records overwrite the
      // hand-over rows once every neighbour has read them.
      nlp_phase_sync();
      if (lane == 0 && i0 > 0) {                            // this chunk's first node for the chunk below
#pragma unroll
        for (int k = 0; k < UPN; ++k) lds_up[64 * UPN + k] = upv[k];
      }
      if (live) {
#pragma unroll
        for (int k = 0; k < SIN_N; ++k) pb.lds[(size_t)i * NLP_BCR_STRIDE + k] = sinv[k];
      }
      nlp_phase_sync();
      continue;
    }
    if (live) {
#pragma unroll
      for (int k = 0; k < SIN_N; ++k) lds_rec[lane * NLP_REC_STRIDE + k] = sinv[k];
    }
    nlp_phase_sync();
    if (lane == 0) {                                        // this chunk's first node for the chunk below
#pragma unroll
      for (int k = 0; k < UPN; ++k) lds_up[64 * UPN + k] = upv[k];
    }
    if constexpr (FREE) {                                   // D' and E' also into the second set of records (its t' slots: above)
      const int cnt = (N - i0 < 64 ? N - i0 : 64) * SIN_N;
      double *dst = pb.ws + (size_t)WS_SIN * N + (size_t)i0 * SIN_N, *dst2 = pb.ws + (size_t)WSF_SIN2 * N + (size_t)i0 * SIN_N;
      for (int e = lane; e < cnt; e += 64) {
        const int node = e / SIN_N, k = e - node * SIN_N;
        const double v = lds_rec[node * NLP_REC_STRIDE + k];
        dst[e] = v;
        if (k < SIN_T) dst2[e] = v;
      }
    } else
    {
      const int cnt = (N - i0 < 64 ? N - i0 : 64) * SIN_N;
      double *dst = pb.ws + (size_t)WS_SIN * N + (size_t)i0 * SIN_N;
      for (int e = lane; e < cnt; e += 64) {
        const int node = e / SIN_N;
        dst[e] = lds_rec[node * NLP_REC_STRIDE + (e - node * SIN_N)];
      }
    }
    nlp_phase_sync();
  }
  *pd_out = __builtin_amdgcn_ballot_w64(bad != 0) == 0ull;
  if constexpr (FREE) { fr_out->gu = rho * wave_sum(gu); fr_out->dd = rho * wave_sum(dd); }
  return wave_max(err);
}

// The Newton system  M dw = rhs / 2  (M: block tridiagonal, 5x5 blocks D_i + damping, sub-diagonal blocks E_i whose only
// non-zero columns are x, y, psi of node i-1).  phi_i and v_i are coupled to (x, y, psi) of nodes i and i-1 only and to no
// other node's phi, v: they are eliminated NODE BY NODE IN PARALLEL (2x2 Cholesky + Schur complement), which leaves a block
// tridiagonal system with 3x3 blocks in (x, y, psi) for the serial recursion -- 80 instead of 280 fp64 operations per node on
// the serial chain.
// The elimination itself is the tail of nlp_assemble (the blocks are in registers there); what remains is the hand-over between
// neighbours (lane = node):  D'_i -= (Rt^T Rt)_{i+1},  t'_i -= (Rt^T tt)_{i+1}.

// The two serial recursions, TWISTED: the block Cholesky runs from both ends of the horizon towards the middle node m = N/2 at
// the same time -- lanes 0..31 eliminate nodes 0, 1, .. m-1, lanes 32..63 nodes N-1, N-2, .. m+1, one instruction stream (inside a
// half every lane computes and stores the same values) -- and the back substitution runs from the middle outwards the same way:
// the dependent chain is N/2 nodes long instead of N.
//   step of a half:  Lo = C Lp^-T,  S = D' - Lo Lo^T,  L = chol(S),  y = L^-1 (t' - Lo yp)
//   C = block (this node, node eliminated before it): E'_i for the lower half, E'_{i+1}^T for the upper half
//   middle:          S_m = D'_m - Lo Lo^T (from m-1) - Uo Uo^T (from m+1),  y_m = L_m^-1 (t'_m - Lo y_{m-1} - Uo y_{m+1})
//   back:            d_m = L_m^-T y_m;  d_i = L_i^-T (y_i - Lon^T dn)  with Lon, dn of the node next to i on the middle's side
// Own functions, not inlined (inside the solver's loop nest the compiler spilled a dozen scalar registers around every node);
// global address space stated explicitly (through a generic pointer the loads would be FLAT ones, whose waits also wait for the
// stores); a ring of four node buffers with the loop unrolled by four (the node three steps ahead is requested before a node is
// processed: one node's arithmetic is shorter than an L2 round trip, and no buffer is ever copied); every lane of a half stores the
// same values to the same address (a store under `if (lane == 0)` sits behind a branch, and the wait for the next loads then
// also waits for the stores: vmcnt counts in order and the compiler cannot count through a branch); a full wait before each
// loop so that the loop-head wait is the back edge's.
struct NlpNodeIn {
  double v[SIN_N];
};

__device__ __forceinline__ double nlp_other_half(double v) {              // the value the lane 32 places away holds
  return __hiloint2double(__builtin_amdgcn_ds_bpermute(((threadIdx.x ^ 32) & 63) << 2, __double2hiint(v)),
                          __builtin_amdgcn_ds_bpermute(((threadIdx.x ^ 32) & 63) << 2, __double2loint(v)));
}

// one elimination step from the reduced node `in` (D' 6, C 9 row-major, t' 3) and the factor (Lp, yp) of the node before it
__device__ __forceinline__ void nlp_block_lo(const double (&C)[3][3], const double (&Lp)[6], double (&Lo)[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double v = C[a][c];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= Lp[c * (c + 1) / 2 + k] * Lo[a][k];
      Lo[a][c] = v * Lp[c * (c + 1) / 2 + c];             // (the diagonal slots hold 1 / L_cc; first node of a half: Lp = 0 -> Lo = 0)
    }
  }
}
__device__ __forceinline__ bool nlp_block_chol(const double (&S)[6], const double (&t)[3], double (&L)[6], double (&y)[3]) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int c = 0; c <= a; ++c) {
      double v = S[a * (a + 1) / 2 + c];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= L[a * (a + 1) / 2 + k] * L[c * (c + 1) / 2 + k];
      if (a == c) {
        if (!(v > 0.0)) { ok = false; v = 1.0; }
        L[a * (a + 1) / 2 + a] = nlp_rsqrt(v);             // the factor keeps the RECIPROCAL diagonal: every later use divides by it
      } else {
        L[a * (a + 1) / 2 + c] = v * L[c * (c + 1) / 2 + c];
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double v = t[a];
#pragma unroll
    for (int k = 0; k < a; ++k) v -= L[a * (a + 1) / 2 + k] * y[k];
    y[a] = v * L[a * (a + 1) / 2 + a];
  }
  return ok;
}


typedef __attribute__((address_space(1))) double gdouble;
// ---- the reduced system by BLOCK CYCLIC REDUCTION (round 3) ----------------------------------------------------------------
// The block-tridiagonal system of the reduced nodes (3x3 blocks D'_i, E'_i = block (i, i-1), right-hand sides t'_i) is symmetric
// positive definite when the step is usable, so any elimination order is a Cholesky factorisation of it.  Odd-even order: at the
// level of stride s the nodes j = s (2m + 1) are eliminated ALL AT ONCE, one lane per node, against their neighbours a = j - s and
// b = j + s, which survive with
//     D_a -= E_j^T P_j,  t_a -= E_j^T r_j;      D_b -= E_b Q_j,  t_b -= E_b r_j,  E_b <- -E_b P_j  (now block (b, a))
//     P_j = D_j^-1 E_j,  Q_j = D_j^-1 E_b^T,  r_j = D_j^-1 t_j
// and after ceil(log2 N) levels node 0 is alone; the unknowns come back level by level, x_j = r_j - P_j x_a - Q_j x_b.  The
// twisted recursion it replaces is a dependent chain of N/2 block pivots (88 k + 27 k of the 200 k cycles of a Newton step at
// N = 121); this is 7 levels of independent 3x3 work.  A node has one left and one right producer per level: the producers apply
// their update to the left neighbour first, then (after a wave-level sync) to the right one, so no two lanes touch a record at once.
// Up to NLP_BCR_LDS_NODES nodes the records live in the wave's LDS (stride 19), P_j and Q_j take the place of the eliminated
// node's record and x_j that of P_j; longer horizons run the same code on the records in global memory.
__device__ __forceinline__ void nlp_solve3(const double (&L)[6], const double b0, const double b1, const double b2, double &x0, double &x1, double &x2) {
  // L L^T x = b with the factor of nlp_block_chol (reciprocal diagonal)
  const double y0 = b0 * L[0];
  const double y1 = (b1 - L[1] * y0) * L[2];
  const double y2 = (b2 - L[3] * y0 - L[4] * y1) * L[5];
  x2 = y2 * L[5];
  x1 = (y1 - L[4] * x2) * L[2];
  x0 = (y0 - L[1] * x1 - L[3] * x2) * L[0];
}

// RT: pointer type of the records -- LDS (address space 3) or global (1): stated, so that the accesses are ds_ / global_ instructions
// (through generic pointers they were flat_ ones: 51 k cycles per Newton step instead of the 30 k of this version)
typedef __attribute__((address_space(3))) double ldouble;
template <typename RT, bool in_lds>
__device__ __attribute__((noinline)) bool nlp_bcr_t(double *sin_generic, double *sf_generic, double *ds_generic, double *lds_generic, int N,
                                                    bool preloaded) {
  const int lane = threadIdx.x & 63;
  gdouble *sin_g = (gdouble *)sin_generic;
  gdouble *ds_g = (gdouble *)ds_generic;
  RT *lds = (RT *)lds_generic;
  RT *rec = in_lds ? (RT *)lds_generic : (RT *)sin_generic;      // records [node][rs]: D' (6), E' (9), t' (3)
  constexpr int rs = in_lds ? NLP_BCR_STRIDE : SIN_N;
  RT *pq = in_lds ? (RT *)lds_generic : (RT *)sf_generic;        // P (9), Q (9) of an eliminated node [node][ps]
  constexpr int ps = in_lds ? NLP_BCR_STRIDE : SF_N;
  if (in_lds && !preloaded) {
    // (batches of 12 rows of 64: every load of a batch is in flight before its first LDS store -- as a plain loop the compiler waited
    // for each load before storing it, 34 memory round trips in a row at 121 nodes, the longest serial stretch of a Newton step)
    const int total = N * SIN_N;
    for (int e0 = 0; e0 < total; e0 += 12 * 64) {
      double v[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) { const int e = e0 + q * 64 + lane; v[q] = e < total ? (double)sin_g[e] : 0.0; }
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        const int e = e0 + q * 64 + lane;
        const int node = e / SIN_N;
        if (e < total) lds[node * NLP_BCR_STRIDE + (e - node * SIN_N)] = v[q];
      }
    }
    nlp_phase_sync();
  }
  int bad = 0;
  int s = 1;
  for (; s < N; s <<= 1) {
    const int n_el = (N - 1 - s) / (2 * s) + 1;       // eliminated nodes of this level: j = s (2m + 1) < N
    for (int m0 = 0; m0 < n_el; m0 += 64) {
      const int m = m0 + lane;
      const bool act = m < n_el;
      const int j = act ? s * (2 * m + 1) : s, a = j - s, b = j + s;
      const bool has_b = act && b < N;
      double D[6], E[3][3], t[3], Eb[3][3], L[6], y[3], P[3][3], Q[3][3], r[3];
      const RT *pj = rec + (size_t)j * rs, *pb = rec + (size_t)(has_b ? b : j) * rs;
#pragma unroll
      for (int q = 0; q < 6; ++q) D[q] = pj[SIN_D + q];
#pragma unroll
      for (int q = 0; q < 9; ++q) { E[q / 3][q % 3] = pj[SIN_E + q]; Eb[q / 3][q % 3] = has_b ? pb[SIN_E + q] : 0.0; }
#pragma unroll
      for (int q = 0; q < 3; ++q) t[q] = pj[SIN_T + q];
      const bool ok = nlp_block_chol(D, t, L, y);
      if (act && !ok) bad = 1;
      nlp_solve3(L, t[0], t[1], t[2], r[0], r[1], r[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        nlp_solve3(L, E[0][k], E[1][k], E[2][k], P[0][k], P[1][k], P[2][k]);           // column k of E_j
        nlp_solve3(L, Eb[k][0], Eb[k][1], Eb[k][2], Q[0][k], Q[1][k], Q[2][k]);        // column k of E_b^T = row k of E_b
      }
      // the left neighbour: D_a -= E_j^T P_j, t_a -= E_j^T r_j
      if (act) {
        RT *pa = rec + (size_t)a * rs;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
#pragma unroll
          for (int v = 0; v <= u; ++v)
            pa[SIN_D + u * (u + 1) / 2 + v] -= E[0][u] * P[0][v] + E[1][u] * P[1][v] + E[2][u] * P[2][v];
          pa[SIN_T + u] -= E[0][u] * r[0] + E[1][u] * r[1] + E[2][u] * r[2];
        }
      }
      nlp_phase_sync();
      // the right neighbour: D_b -= E_b Q_j, t_b -= E_b r_j, E_b <- -E_b P_j
      if (has_b) {
        RT *pbw = rec + (size_t)b * rs;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
#pragma unroll
          for (int v = 0; v <= u; ++v)
            pbw[SIN_D + u * (u + 1) / 2 + v] -= Eb[u][0] * Q[0][v] + Eb[u][1] * Q[1][v] + Eb[u][2] * Q[2][v];
          pbw[SIN_T + u] -= Eb[u][0] * r[0] + Eb[u][1] * r[1] + Eb[u][2] * r[2];
#pragma unroll
          for (int v = 0; v < 3; ++v) pbw[SIN_E + u * 3 + v] = -(Eb[u][0] * P[0][v] + Eb[u][1] * P[1][v] + Eb[u][2] * P[2][v]);
        }
      }
      // what the way back needs of node j: P_j, Q_j (in place of its record / in the factor's workspace), r_j (in the step's slot)
      if (act) {
        RT *o = pq + (size_t)j * ps;
#pragma unroll
        for (int q = 0; q < 9; ++q) { o[q] = P[q / 3][q % 3]; o[9 + q] = Q[q / 3][q % 3]; }
#pragma unroll
        for (int q = 0; q < 3; ++q) ds_g[(size_t)j * 3 + q] = r[q];
      }
      nlp_phase_sync();
    }
  }
  if (__builtin_amdgcn_ballot_w64(bad != 0) != 0ull) return false;
  // node 0 alone
  {
    double D[6], t[3], L[6], y[3], x[3];
#pragma unroll
    for (int q = 0; q < 6; ++q) D[q] = rec[SIN_D + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = rec[SIN_T + q];
    if (!nlp_block_chol(D, t, L, y)) return false;
    nlp_solve3(L, t[0], t[1], t[2], x[0], x[1], x[2]);
    nlp_phase_sync();
    // (every lane stores the same values: no branch between the loads above and these stores)
#pragma unroll
    for (int q = 0; q < 3; ++q) { ds_g[q] = x[q]; if (in_lds) lds[q] = x[q]; }
    nlp_phase_sync();
  }
  // the way back: the unknowns of a level from those of the coarser ones (in the LDS path x_j takes the place of P_j)
  const RT *xs = in_lds ? (const RT *)lds_generic : (const RT *)ds_generic;
  constexpr int xst = in_lds ? NLP_BCR_STRIDE : 3;
  // LDS path (one chunk per level: N <= 121): r_j sits in global memory -- the only global read of a level, a round trip of its own
  // on the serial chain of seven levels.  The lane that will need r_j of the NEXT level is known (node s/2 (2 lane + 1)): its three
  // values are requested one level ahead and arrive behind the current level's arithmetic.
  double rn[3] = {0.0, 0.0, 0.0};
  auto request_r = [&](int sl) {
    if (!in_lds || sl < 1) return;
    const int n_l = (N - 1 - sl) / (2 * sl) + 1;
    const int jl = lane < n_l ? sl * (2 * lane + 1) : sl;
#pragma unroll
    for (int u = 0; u < 3; ++u) rn[u] = ds_g[(size_t)jl * 3 + u];
  };
  request_r(s >> 1);
  for (s >>= 1; s >= 1; s >>= 1) {
    const int n_el = (N - 1 - s) / (2 * s) + 1;
    for (int m0 = 0; m0 < n_el; m0 += 64) {
      const int m = m0 + lane;
      const bool act = m < n_el;
      const int j = act ? s * (2 * m + 1) : s, a = j - s, b = j + s;
      const bool has_b = act && b < N;
      double x[3], rj[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) rj[u] = in_lds ? rn[u] : (act ? (double)ds_g[(size_t)j * 3 + u] : 0.0);
      request_r(s >> 1);
      if (act) {
        const RT *o = pq + (size_t)j * ps;
        const RT *xa = xs + (size_t)a * xst, *xb = xs + (size_t)(has_b ? b : a) * xst;
        const double a0 = xa[0], a1 = xa[1], a2 = xa[2];
        const double b0 = has_b ? xb[0] : 0.0, b1 = has_b ? xb[1] : 0.0, b2 = has_b ? xb[2] : 0.0;
#pragma unroll
        for (int u = 0; u < 3; ++u)
          x[u] = rj[u] - (o[u * 3] * a0 + o[u * 3 + 1] * a1 + o[u * 3 + 2] * a2)
                 - (o[9 + u * 3] * b0 + o[9 + u * 3 + 1] * b1 + o[9 + u * 3 + 2] * b2);
      }
      nlp_phase_sync();                       // (every P_j of the chunk has been read before an x_j overwrites one)
      if (act) {
#pragma unroll
        for (int u = 0; u < 3; ++u) { ds_g[(size_t)j * 3 + u] = x[u]; if (in_lds) lds[(size_t)j * NLP_BCR_STRIDE + u] = x[u]; }
      }
      nlp_phase_sync();
    }
  }
  return true;
}
// preloaded: the records are in the LDS block already (nlp_assemble with rec_lds; only for N <= NLP_BCR_LDS_NODES)
__device__ __forceinline__ bool nlp_bcr(double *sin_g, double *sf_g, double *ds_g, double *lds, int N, bool preloaded) {
  if (N <= NLP_BCR_LDS_NODES) return nlp_bcr_t<ldouble, true>(sin_g, sf_g, ds_g, lds, N, preloaded);
  return nlp_bcr_t<gdouble, false>(sin_g, sf_g, ds_g, lds, N, false);
}

// mid: 9 doubles of scratch for the second coupling block of the middle node (its coupling to node m+1)
__device__ __attribute__((noinline)) bool nlp_factor(double *sin_generic, double *sf_generic, double *mid_generic, int N) {
  const gdouble *sin = (const gdouble *)sin_generic;
  gdouble *sf = (gdouble *)sf_generic;
  gdouble *mid = (gdouble *)mid_generic;
  const bool up = (threadIdx.x & 32) != 0;                   // upper half: nodes N-1 down to m+1
  const int m = N >> 1, nlo = m, cnt = up ? N - 1 - m : m;   // (cnt >= 1 for N >= 3; the upper half has nlo or nlo - 1 nodes)
  // inputs of step k of this lane's half: D', t' of its node i; C from E' of node i (lower) / E'^T of node i+1 (upper)
  auto load = [&](int k, NlpNodeIn &n) {
    const int kk = k < cnt ? k : cnt - 1;
    const int i = up ? N - 1 - kk : kk;
    const int ie = up ? (i + 1 < N ? i + 1 : i) : i;
    const gdouble *pd = sin + (long)i * SIN_N, *pe = sin + (long)ie * SIN_N;
#pragma unroll
    for (int q = 0; q < 6; ++q) n.v[SIN_D + q] = pd[SIN_D + q];
#pragma unroll
    for (int q = 0; q < 9; ++q) n.v[SIN_E + q] = pe[SIN_E + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) n.v[SIN_T + q] = pd[SIN_T + q];
  };
  auto coupling = [&](const NlpNodeIn &n, bool zero, double (&C)[3][3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = up ? n.v[SIN_E + c * 3 + a] : n.v[SIN_E + a * 3 + c];
        C[a][c] = zero ? 0.0 : v;
      }
  };
  double Lp[6], yp[3];                         // factor of the node eliminated before (reciprocal diagonal), its y
#pragma unroll
  for (int k = 0; k < 6; ++k) Lp[k] = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) yp[c] = 0.0;
  bool ok = true;
  NlpNodeIn buf[4];
  load(0, buf[0]); load(1, buf[1]); load(2, buf[2]);
  __builtin_amdgcn_s_waitcnt(0x0F70);                        // vmcnt(0)
  for (int k0 = 0; k0 < nlo; k0 += 4) {
#pragma unroll
   for (int u = 0; u < 4; ++u) {
    const int k = k0 + u;
    if (k >= nlo) break;
    load(k + 3, buf[(u + 3) & 3]);
    const NlpNodeIn &cur = buf[u];
    if (k < cnt) {                                           // (the upper half may be one node shorter)
      const int i = up ? N - 1 - k : k;
      double C[3][3], Lo[3][3], S[6], t[3], L[6], y[3];
      coupling(cur, k == 0, C);                              // (first node of a half: nothing before it)
      nlp_block_lo(C, Lp, Lo);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c <= a; ++c)
          S[a * (a + 1) / 2 + c] = cur.v[SIN_D + a * (a + 1) / 2 + c] - (Lo[a][0] * Lo[c][0] + Lo[a][1] * Lo[c][1] + Lo[a][2] * Lo[c][2]);
        t[a] = cur.v[SIN_T + a] - (Lo[a][0] * yp[0] + Lo[a][1] * yp[1] + Lo[a][2] * yp[2]);
      }
      ok = nlp_block_chol(S, t, L, y) && ok;
      gdouble *o = sf + (long)i * SF_N;
#pragma unroll
      for (int q = 0; q < 6; ++q) o[SF_L + q] = L[q];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[SF_LO + a * 3 + c] = Lo[a][c];
#pragma unroll
      for (int a = 0; a < 3; ++a) o[SF_Y + a] = y[a];
#pragma unroll
      for (int q = 0; q < 6; ++q) Lp[q] = L[q];
#pragma unroll
      for (int a = 0; a < 3; ++a) yp[a] = y[a];
    }
   }
  }
  // ---- the middle node: both halves hand in their Schur complement
  {
    NlpNodeIn md;
    const int ie = up ? m + 1 : m;
    const gdouble *pd = sin + (long)m * SIN_N, *pe = sin + (long)ie * SIN_N;
#pragma unroll
    for (int q = 0; q < 6; ++q) md.v[SIN_D + q] = pd[SIN_D + q];
#pragma unroll
    for (int q = 0; q < 9; ++q) md.v[SIN_E + q] = pe[SIN_E + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) md.v[SIN_T + q] = pd[SIN_T + q];
    double C[3][3], Lo[3][3], S[6], t[3], L[6], y[3];
    coupling(md, false, C);
    nlp_block_lo(C, Lp, Lo);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int c = 0; c <= a; ++c) {
        const double p = Lo[a][0] * Lo[c][0] + Lo[a][1] * Lo[c][1] + Lo[a][2] * Lo[c][2];
        S[a * (a + 1) / 2 + c] = md.v[SIN_D + a * (a + 1) / 2 + c] - (p + nlp_other_half(p));
      }
      const double q = Lo[a][0] * yp[0] + Lo[a][1] * yp[1] + Lo[a][2] * yp[2];
      t[a] = md.v[SIN_T + a] - (q + nlp_other_half(q));
    }
    ok = nlp_block_chol(S, t, L, y) && ok;
    gdouble *o = sf + (long)m * SF_N;
#pragma unroll
    for (int q = 0; q < 6; ++q) o[SF_L + q] = L[q];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[SF_Y + a] = y[a];
    gdouble *oc = up ? mid : o + SF_LO;                      // coupling to m-1 with the node, coupling to m+1 in the scratch
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) oc[a * 3 + c] = Lo[a][c];
  }
  return __builtin_amdgcn_ballot_w64(!ok) == 0ull;
}

// Serial recursion 2, from the middle outwards in both halves: ds_m = L_m^-T y_m;  ds_i = L_i^-T (y_i - Lon^T dn).
// VIA: vm the fixed set of the nodes; a node's mask travels in the ring with its factor record, and the middle node can be pinned too.
typedef __attribute__((address_space(1))) int32_t gint32;
template <bool VIA = false>
__device__ __attribute__((noinline)) void nlp_backsolve(double *sf_generic, double *mid_generic, double *ds_generic, int N,
                                                        const int32_t *vm_generic = nullptr) {
  const gdouble *sf = (const gdouble *)sf_generic;
  [[maybe_unused]] const gint32 *vm = (const gint32 *)vm_generic;
  const gdouble *mid = (const gdouble *)mid_generic;
  gdouble *dsv = (gdouble *)ds_generic;
  const bool up = (threadIdx.x & 32) != 0;
  const int m = N >> 1, nlo = m, cnt = up ? N - 1 - m : m;
  auto node_of = [&](int k) { const int kk = k < cnt ? k : cnt - 1; return up ? m + 1 + kk : m - 1 - kk; };
  NlpNodeIn buf[4];
  [[maybe_unused]] int mk[4] = {0, 0, 0, 0};
  auto load = [&](int k, int slot) {                        // slot: the ring position, a compile-time value at every call
    NlpNodeIn &n = buf[slot];
    const gdouble *p = sf + (long)node_of(k) * SF_N;
#pragma unroll
    for (int q = 0; q < SF_N; ++q) n.v[q] = p[q];
    if constexpr (VIA) mk[slot] = vm[node_of(k)];
  };
  auto subst = [&](const double *v, const double (&t)[3], double (&ds)[3]) {       // ds = L^-T t (v: the node's factor record)
#pragma unroll
    for (int a = 2; a >= 0; --a) {
      double x = t[a];
#pragma unroll
      for (int k = a + 1; k < 3; ++k) x -= v[SF_L + k * (k + 1) / 2 + a] * ds[k];
      ds[a] = x * v[SF_L + a * (a + 1) / 2 + a];
    }
  };
  load(0, 0); load(1, 1); load(2, 2);
  double dn[3], Lon[3][3];
  {
    NlpNodeIn md;
    const gdouble *p = sf + (long)m * SF_N;
#pragma unroll
    for (int q = 0; q < SF_N; ++q) md.v[q] = p[q];
    const gdouble *pc = up ? mid : p + SF_LO;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) Lon[a][c] = pc[a * 3 + c];
    [[maybe_unused]] int mm = 0;
    if constexpr (VIA) mm = vm[m];
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0)
    double t[3] = {md.v[SF_Y], md.v[SF_Y + 1], md.v[SF_Y + 2]};
    subst(md.v, t, dn);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (VIA) { if ((mm >> c) & 1) dn[c] = 0.0; }
      dsv[(long)m * 3 + c] = dn[c];
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);
  for (int k0 = 0; k0 < nlo; k0 += 4) {
#pragma unroll
   for (int u = 0; u < 4; ++u) {
    const int k = k0 + u;
    if (k >= nlo) break;
    load(k + 3, (u + 3) & 3);
    const NlpNodeIn &cur = buf[u];
    if (k < cnt) {
      const int i = up ? m + 1 + k : m - 1 - k;
      double t[3], ds[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) t[a] = cur.v[SF_Y + a] - (Lon[0][a] * dn[0] + Lon[1][a] * dn[1] + Lon[2][a] * dn[2]);
      subst(cur.v, t, ds);
      const bool fx = i == 0 || i == N - 1;                 // end conditions: fixed variables
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if constexpr (VIA) { if ((mk[u] >> c) & 1) ds[c] = 0.0; }
        else
        if (fx) ds[c] = 0.0;
        dn[c] = ds[c];
        dsv[(long)i * 3 + c] = ds[c];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) Lon[a][c] = cur.v[SF_LO + a * 3 + c];
    }
   }
  }
}

// Recovery of the eliminated (phi, v) steps + step statistics (node-parallel): d(phi, v)_i = LP^-T (tt - Qt ds_i - Rt ds_{i-1});
// directional derivative of the merit function, largest primal step (fraction to the boundary) and the dual steps' largest
// fraction.  Wave-uniform results.
// KEEP: g is quadratic in the step, g(a) = g + 2 a d.s + a^2 |s|^2 with s the step of (x, y): the fraction-to-the-boundary rule
// g(a) >= (1 - tau) g is the smaller positive root of  |s|^2 a^2 + 2 (d.s) a + tau g = 0  (none when d.s >= 0 or the discriminant is not
// positive), in the form tau g / (sqrt(disc) - d.s) that does not cancel; the dual's step is dz = mub / g - z - (z / g) 2 d.s.  The
// directional derivative needs nothing: the right-hand side carries the discs' terms.
// FENCE: g is linear in the step, g(a) = g - a (a . s): the rule is a <= tau g / (a . s) where a . s > 0, taken like a box bound's; the
// dual's step is dz = (mub + z a . s) / g - z.
template <unsigned F>
__device__ void nlp_recover_stats(const NlpProbV<F> &pb, const NlpScen &s, int lane, double mub, double tau, double *dphi_out,
                                  double *amax_out, double *az_out) {
  NLP_FEATURES(F);
  const int N = pb.N;
  double dphi = 0.0, amax = 1.0, az = 1.0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i >= N) continue;
    // (all loads of the node up front: see nlp_merit)
    const int im = i >= 1 ? i - 1 : 0;
    double dwv[NLP_NV], dsp[3], wv[NLP_NV], rhv[NLP_NV], zlv[NLP_NV], zuv[NLP_NV], elq[6], elr[6], ellp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { dwv[c] = NLP_DS(c, i); dsp[c] = NLP_DS(c, im); }
    if (i < 1) { dsp[0] = 0.0; dsp[1] = 0.0; dsp[2] = 0.0; }
    double z0 = NLP_EL(EL_T + 0, i), z1 = NLP_EL(EL_T + 1, i);
#pragma unroll
    for (int k = 0; k < 6; ++k) { elq[k] = NLP_EL(EL_Q + k, i); elr[k] = NLP_EL(EL_R + k, i); }
#pragma unroll
    for (int k = 0; k < 3; ++k) ellp[k] = NLP_EL(EL_LP + k, i);
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) { wv[c] = NLP_W(c, i); rhv[c] = NLP_RHS(c, i); zlv[c] = NLP_P(WS_ZL + c, i); zuv[c] = NLP_P(WS_ZU + c, i); }
    [[maybe_unused]] const int vmi = nlp_via_mask<F>(pb, i);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      z0 -= elq[k] * dwv[k] + elr[k] * dsp[k];
      z1 -= elq[3 + k] * dwv[k] + elr[3 + k] * dsp[k];
    }
    dwv[4] = z1 * ellp[2];
    dwv[3] = (z0 - ellp[1] * dwv[4]) * ellp[0];
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) {
      const double dw = dwv[c];
      NLP_DW(c, i) = dw;
      dphi -= rhv[c] * dw;
      if (nlp_fixed_at<F>(i, N, c, vmi)) continue;
      const double w = wv[c];
      if (s.lo[c] > -1e299) {
        const double sl = w - s.lo[c], z = zlv[c];
        if (-dw * amax > tau * sl) amax = -tau * sl / dw;          // (divide only when the bound is the binding one so far)
        const double dz = (mub - z * dw) / sl - z;
        if (-dz * az > tau * z) az = -tau * z / dz;
      }
      if (s.hi[c] < 1e299) {
        const double su = s.hi[c] - w, z = zuv[c];
        if (dw * amax > tau * su) amax = tau * su / dw;
        const double dz = (mub + z * dw) / su - z;
        if (-dz * az > tau * z) az = -tau * z / dz;
      }
    }
    if constexpr (KEEP) {
      if (i >= 1 && i < N - 1) {
        const double *__restrict__ dk = pb.keep.discs;
        const double aa = KMOV ? nlp_dot2(dwv[0], dwv[0], dwv[1], dwv[1]) : dwv[0] * dwv[0] + dwv[1] * dwv[1];
#pragma clang loop unroll(disable)
        for (int m = 0; m < pb.keep.n; ++m) {
          [[maybe_unused]] double cxm = 0.0, cym = 0.0;
          if constexpr (KMOV) { cxm = pb.keep.ctr[(size_t)(2 * m) * N + i]; cym = pb.keep.ctr[(size_t)(2 * m + 1) * N + i]; }
          const double R = dk[KMOV ? 2 * m : 3 * m + 2];
          if (!(R > 0.0)) continue;
          const double dx = wv[0] - (KMOV ? cxm : dk[3 * m]), dy = wv[1] - (KMOV ? cym : dk[3 * m + 1]);
          const double gk = KMOV ? nlp_keep_g(dx, dy, R) : dx * dx + dy * dy - R * R, z = pb.keep.z[(size_t)m * N + i];
          const double bh = KMOV ? nlp_dot2(dx, dwv[0], dy, dwv[1]) : dx * dwv[0] + dy * dwv[1];
          if (bh < 0.0) {
            const double cq = tau * gk, disc = KMOV ? fma(bh, bh, -(aa * cq)) : bh * bh - aa * cq;
            if (disc > 0.0) amax = fmin(amax, cq / (sqrt(disc) - bh));
          }
          const double dz = (mub - 2.0 * z * bh) / gk - z;
          if (-dz * az > tau * z) az = -tau * z / dz;
        }
      }
    }
    if constexpr (FENCE) {
      if (i >= 1 && i < N - 1) {
#pragma clang loop unroll(disable)
        for (int k = 0; k < pb.fence.n; ++k) {
          const double *__restrict__ e = pb.fence.edges + 4 * k;
          if (!nlp_fence_present(e)) continue;
          const double gk = nlp_fence_g(e, wv[0], wv[1]), z = pb.fence.z[(size_t)k * N + i], as = nlp_dot2(e[0], dwv[0], e[1], dwv[1]);
          if (as * amax > tau * gk) amax = tau * gk / as;
          const double dz = fma(z, as, mub) / gk - z;
          if (-dz * az > tau * z) az = -tau * z / dz;
        }
      }
    }
  }
  *dphi_out = wave_sum(dphi); *amax_out = wave_min(amax); *az_out = wave_min(az);
}

// FREE: nlp_recover_stats for the bordered system  [A b; b^T d] (dW, du) = (r, r_u) / 2  by the Schur complement on d.  The two
// passes of the cyclic reduction left the reduced parts of x0 = A^-1 r / 2 (WS_DS) and y = A^-1 b (WSF_DS2); the first pass here
// recovers (phi, v) of both, node-parallel, keeps x0 in the step's planes and y in its own, and sums b.x0 and b.y; then
//   du = (r_u / 2 - b.x0) / (d - b.y),   dW = x0 - y du
// and the second pass is nlp_recover_stats' own: directional derivative and the two ratio tests, with u and its duals included.
// false: d - b.y is not positive -- the bordered matrix is not positive definite (the caller raises the damping).
// KEEP, FENCE: the second pass takes the families' ratio tests and dual steps of nlp_recover_stats behind the box's, discs then edges,
// ahead of u's: the order of oracle.nlp.solve_general.  The first pass does not change: b holds nothing of them.
template <unsigned F>
__device__ bool nlp_recover_free(const NlpProbT<F> &pb, const NlpScen &s, int lane, double mub, double tau, double ru, double d,
                                 double *dphi_out, double *amax_out, double *az_out, double *du_out) {
  NLP_FEATURES(F);
  const int N = pb.N;
  double bx = 0.0, by = 0.0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i >= N) continue;
    const int im = i >= 1 ? i - 1 : 0;
    double xv[NLP_NV], yv[NLP_NV], xp[3], yp[3], bvv[NLP_NV], elq[6], elr[6], ellp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xv[c] = NLP_DS(c, i); xp[c] = NLP_DS(c, im);
      yv[c] = pb.ws[(size_t)WSF_DS2 * N + i * 3 + c]; yp[c] = pb.ws[(size_t)WSF_DS2 * N + im * 3 + c];
    }
    if (i < 1) { xp[0] = 0.0; xp[1] = 0.0; xp[2] = 0.0; yp[0] = 0.0; yp[1] = 0.0; yp[2] = 0.0; }
    double z0 = NLP_EL(EL_T + 0, i), z1 = NLP_EL(EL_T + 1, i), q0 = NLP_P(WSF_TB + 0, i), q1 = NLP_P(WSF_TB + 1, i);
#pragma unroll
    for (int k = 0; k < 6; ++k) { elq[k] = NLP_EL(EL_Q + k, i); elr[k] = NLP_EL(EL_R + k, i); }
#pragma unroll
    for (int k = 0; k < 3; ++k) ellp[k] = NLP_EL(EL_LP + k, i);
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) bvv[c] = NLP_P(WSF_B + c, i);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      z0 -= elq[k] * xv[k] + elr[k] * xp[k];
      z1 -= elq[3 + k] * xv[k] + elr[3 + k] * xp[k];
      q0 -= elq[k] * yv[k] + elr[k] * yp[k];
      q1 -= elq[3 + k] * yv[k] + elr[3 + k] * yp[k];
    }
    xv[4] = z1 * ellp[2]; xv[3] = (z0 - ellp[1] * xv[4]) * ellp[0];
    yv[4] = q1 * ellp[2]; yv[3] = (q0 - ellp[1] * yv[4]) * ellp[0];
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) {
      NLP_DW(c, i) = xv[c]; NLP_P(WSF_Y + c, i) = yv[c];
      bx += bvv[c] * xv[c]; by += bvv[c] * yv[c];
    }
  }
  bx = wave_sum(bx); by = wave_sum(by);
  const double sch = d - by;
  if (!(sch > 0.0)) return false;
  const double du = (0.5 * ru - bx) / sch;
  double dphi = 0.0, amax = 1.0, az = 1.0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i >= N) continue;
    double xv[NLP_NV], yv[NLP_NV], wv[NLP_NV], rhv[NLP_NV], zlv[NLP_NV], zuv[NLP_NV];
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) {
      xv[c] = NLP_DW(c, i); yv[c] = NLP_P(WSF_Y + c, i);        // (this lane's own stores of the pass above)
      wv[c] = NLP_W(c, i); rhv[c] = NLP_RHS(c, i); zlv[c] = NLP_P(WS_ZL + c, i); zuv[c] = NLP_P(WS_ZU + c, i);
    }
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) {
      const double dw = xv[c] - yv[c] * du;
      NLP_DW(c, i) = dw;
      dphi -= rhv[c] * dw;
      if (nlp_fixed(i, N, c)) continue;
      const double w = wv[c];
      if (s.lo[c] > -1e299) {
        const double sl = w - s.lo[c], z = zlv[c];
        if (-dw * amax > tau * sl) amax = -tau * sl / dw;
        const double dz = (mub - z * dw) / sl - z;
        if (-dz * az > tau * z) az = -tau * z / dz;
      }
      if (s.hi[c] < 1e299) {
        const double su = s.hi[c] - w, z = zuv[c];
        if (dw * amax > tau * su) amax = tau * su / dw;
        const double dz = (mub + z * dw) / su - z;
        if (-dz * az > tau * z) az = -tau * z / dz;
      }
    }
    if constexpr (KEEP) {
      if (i >= 1 && i < N - 1) {
        const double *__restrict__ dk = pb.keep.discs;
        const double sx = xv[0] - yv[0] * du, sy = xv[1] - yv[1] * du, aa = sx * sx + sy * sy;
#pragma clang loop unroll(disable)
        for (int m = 0; m < pb.keep.n; ++m) {
          const double R = dk[3 * m + 2];
          if (!(R > 0.0)) continue;
          const double dx = wv[0] - dk[3 * m], dy = wv[1] - dk[3 * m + 1];
          const double gk = dx * dx + dy * dy - R * R, z = pb.keep.z[(size_t)m * N + i], bh = dx * sx + dy * sy;
          if (bh < 0.0) {
            const double cq = tau * gk, disc = bh * bh - aa * cq;
            if (disc > 0.0) amax = fmin(amax, cq / (sqrt(disc) - bh));
          }
          const double dz = (mub - 2.0 * z * bh) / gk - z;
          if (-dz * az > tau * z) az = -tau * z / dz;
        }
      }
    }
    if constexpr (FENCE) {
      if (i >= 1 && i < N - 1) {
        const double sx = xv[0] - yv[0] * du, sy = xv[1] - yv[1] * du;
#pragma clang loop unroll(disable)
        for (int k = 0; k < pb.fence.n; ++k) {
          const double *__restrict__ e = pb.fence.edges + 4 * k;
          if (!nlp_fence_present(e)) continue;
          const double gk = nlp_fence_g(e, wv[0], wv[1]), z = pb.fence.z[(size_t)k * N + i], as = nlp_dot2(e[0], sx, e[1], sy);
          if (as * amax > tau * gk) amax = tau * gk / as;
          const double dz = fma(z, as, mub) / gk - z;
          if (-dz * az > tau * z) az = -tau * z / dz;
        }
      }
    }
  }
  dphi = wave_sum(dphi) - ru * du; amax = wave_min(amax); az = wave_min(az);
  {
    const double sl = pb.u - pb.ulo, su = pb.uhi - pb.u;
    if (-du * amax > tau * sl) amax = -tau * sl / du;
    if (du * amax > tau * su) amax = tau * su / du;
    const double dzl = (mub - pb.zul * du) / sl - pb.zul, dzu = (mub + pb.zuu * du) / su - pb.zuu;
    if (-dzl * az > tau * pb.zul) az = -tau * pb.zul / dzl;
    if (-dzu * az > tau * pb.zuu) az = -tau * pb.zuu / dzu;
  }
  *dphi_out = dphi; *amax_out = amax; *az_out = az; *du_out = du;
  return true;
}

// Take the step (node-parallel): W += a dw, duals += az dz (dz from the step's dw), duals kept near the central path.
// KEEP: the discs' duals move and are clipped like the box duals, with g at the new point.
// FENCE: the edges' duals likewise.
template <unsigned F>
__device__ void nlp_apply(const NlpProbV<F> &pb, const NlpScen &s, int lane, double a, double az, double mub) {
  NLP_FEATURES(F);
  const int N = pb.N;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i >= N) continue;
    // (all loads of the node up front: see nlp_merit)
    double wv[NLP_NV], dwl[NLP_NV], zlv[NLP_NV], zuv[NLP_NV];
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) { wv[c] = NLP_W(c, i); dwl[c] = NLP_DW(c, i); zlv[c] = NLP_P(WS_ZL + c, i); zuv[c] = NLP_P(WS_ZU + c, i); }
    [[maybe_unused]] const int vmi = nlp_via_mask<F>(pb, i);
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) {
      if (nlp_fixed_at<F>(i, N, c, vmi)) continue;
      const double w = wv[c], dw = dwl[c];
      const double wn = w + a * dw;
      NLP_W(c, i) = wn;
      if (s.lo[c] > -1e299) {
        const double sl = w - s.lo[c], z = zlv[c], mn = mub / (wn - s.lo[c]);
        double zn = z + az * ((mub - z * dw) / sl - z);
        zn = fmin(fmax(zn, 1e-10 * mn), 1e10 * mn);
        NLP_P(WS_ZL + c, i) = zn;
      }
      if (s.hi[c] < 1e299) {
        const double su = s.hi[c] - w, z = zuv[c], mn = mub / (s.hi[c] - wn);
        double zn = z + az * ((mub + z * dw) / su - z);
        zn = fmin(fmax(zn, 1e-10 * mn), 1e10 * mn);
        NLP_P(WS_ZU + c, i) = zn;
      }
    }
    if constexpr (KEEP) {
      if (i >= 1 && i < N - 1) {
        const double *__restrict__ dk = pb.keep.discs;
        const double xn = wv[0] + a * dwl[0], yn = wv[1] + a * dwl[1];
#pragma clang loop unroll(disable)
        for (int m = 0; m < pb.keep.n; ++m) {
          [[maybe_unused]] double cxm = 0.0, cym = 0.0;
          if constexpr (KMOV) { cxm = pb.keep.ctr[(size_t)(2 * m) * N + i]; cym = pb.keep.ctr[(size_t)(2 * m + 1) * N + i]; }
          const double R = dk[KMOV ? 2 * m : 3 * m + 2];
          if (!(R > 0.0)) continue;
          const double dx = wv[0] - (KMOV ? cxm : dk[3 * m]), dy = wv[1] - (KMOV ? cym : dk[3 * m + 1]);
          const double ex = xn - (KMOV ? cxm : dk[3 * m]), ey = yn - (KMOV ? cym : dk[3 * m + 1]);
          const double gk = KMOV ? nlp_keep_g(dx, dy, R) : dx * dx + dy * dy - R * R, gn = KMOV ? nlp_keep_g(ex, ey, R) : ex * ex + ey * ey - R * R;
          const double z = pb.keep.z[(size_t)m * N + i];
          const double bh = KMOV ? nlp_dot2(dx, dwl[0], dy, dwl[1]) : dx * dwl[0] + dy * dwl[1], mn = mub / gn;
          double zn = z + az * ((mub - 2.0 * z * bh) / gk - z);
          zn = fmin(fmax(zn, 1e-10 * mn), 1e10 * mn);
          pb.keep.z[(size_t)m * N + i] = zn;
        }
      }
    }
    if constexpr (FENCE) {
      if (i >= 1 && i < N - 1) {
        const double xn = fma(a, dwl[0], wv[0]), yn = fma(a, dwl[1], wv[1]);      // (the new node, for the clip's bounds only)
#pragma clang loop unroll(disable)
        for (int k = 0; k < pb.fence.n; ++k) {
          const double *__restrict__ e = pb.fence.edges + 4 * k;
          if (!nlp_fence_present(e)) continue;
          const double gk = nlp_fence_g(e, wv[0], wv[1]), gn = nlp_fence_g(e, xn, yn), z = pb.fence.z[(size_t)k * N + i];
          const double as = nlp_dot2(e[0], dwl[0], e[1], dwl[1]), mn = mub / gn;
          double zn = z + az * (fma(z, as, mub) / gk - z);
          zn = fmin(fmax(zn, 1e-10 * mn), 1e10 * mn);
          pb.fence.z[(size_t)k * N + i] = zn;
        }
      }
    }
  }
}

struct NlpOut { double cost, feas; int iters, status; };

// VIA: the pins of one problem -- pts [n][5] = (node, mask, x, y, psi) of d2d_via_points, a row with mask 0 absent -- and vm [N], the
// plane of the nodes' fixed sets that the start pass fills from them.
struct NlpViaSet {
  const double *pts;
  int32_t *vm;
  int n;
};
// The pins of a problem, checked before its solve, one row per lane (n <= D2D_MAX_VIA): a mask that is no integer in 1 .. 7, a node
// that is no integer in 1 .. N-2, a pinned value that is not finite or lies outside the problem's box (the row's, d2d_nlp_opts.bounds
// for psi), or a (node, component) that an earlier row pins already.  Wave-uniform.
__device__ __forceinline__ bool nlp_via_bad(const double *__restrict__ pts, int n, int N, const double *__restrict__ sc, const d2d_nlp_opts &o,
                                            const double *__restrict__ bnd, int lane) {
  const NlpScen s = nlp_load_scen(sc, o, bnd);
  int bad = 0;
  if (lane < n) {
    const double fn = pts[5 * lane], fm = pts[5 * lane + 1];
    if (fm != 0.0) {
      if (!(fm >= 1.0 && fm <= 7.0) || fm != floor(fm) || !(fn >= 1.0 && fn <= (double)(N - 2)) || fn != floor(fn)) {
        bad = 1;
      } else {
        const int m = (int)fm;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double v = pts[5 * lane + 2 + c];
          if ((m >> c) & 1) bad |= !(fabs(v) <= 1.79e308) || v < s.lo[c] || v > s.hi[c];
        }
        for (int e = 0; e < lane; ++e) {
          const double qm = pts[5 * e + 1];
          if (pts[5 * e] == fn && qm >= 1.0 && qm <= 7.0 && ((int)qm & m) != 0) bad = 1;
        }
      }
    }
  }
  return __builtin_amdgcn_ballot_w64(bad != 0) != 0ull;
}

// The optional inputs of nlp_solve_one in one aggregate, so that one call expression serves every instantiation: each reads the
// members of its own feature set and ignores the others (NlpExtra{}: none).  A plain aggregate, initialised in the call expression, on
// purpose: default member initialisers, or a named object whose members are set one by one, moved kernels.
struct NlpExtra {
  NlpModel md;               // MODEL
  const d2d_wind_field *wf;  // WIND: the field and the problem's start time
  double t_start;
  unsigned pmask;            // PAIRS
  const NlpMovSet *mv;       // MOV
  const NlpViaSet *via;      // VIA
  const double *free_row;    // FREE: (h_lo, h_hi, k_dur, h_start; 0 = the launch's h) of the problem, and where its solved h goes
  double *h_out;
  const NlpKeepSet *keep;    // KEEP: the problem's NlpKeepSetT<F> (KMOV: a NlpKeepMovSet, FENCE: a NlpKeepFenceSet)
};

// KEEP: the start of a free node's position.  The box push of the start pass, then every disc in index order, twice (a push out of one
// disc into its neighbour is undone by the second pass): a node with g <= kappa = (1.01^2 - 1) R^2, i.e. closer to the centre than
// 1.01 R, moves radially to |d| = 1.01 R -- along (nx, ny), the left normal of the leg p0 -> p1, where the radial direction is
// degenerate (|d| < 1e-12 R).  The caller re-applies the box push (nlp_box_push), as the start pass does for every variable.
__device__ __forceinline__ double nlp_box_push(double w, double lo, double hi) {
  const bool hl = lo > -1e299, hu = hi < 1e299;
  const double width = (hl && hu) ? hi - lo : 1e300;
  const double kap = fmin(1e-2 * fmax(1.0, fabs(w)), 1e-2 * width);
  if (hl) w = fmax(w, lo + kap);
  if (hu) w = fmin(w, hi - kap);
  return w;
}
// KMOV: the discs' centres are node i's own (N: the planes' stride).
template <unsigned F = NLP_KEEP>
__device__ __forceinline__ void nlp_keep_start(const NlpScen &s, const NlpKeepSetT<F & ~NLP_FENCE> &k, double &x, double &y, [[maybe_unused]] int i = 0, [[maybe_unused]] int N = 0) {
  constexpr bool KMOV = NlpFeatures<F>::KMOV;
  x = nlp_box_push(x, s.lo[0], s.hi[0]); y = nlp_box_push(y, s.lo[1], s.hi[1]);
  const double lx = s.p1[0] - s.p0[0], ly = s.p1[1] - s.p0[1], ll = sqrt(lx * lx + ly * ly);
  const double nx = ll > 0.0 ? -ly / ll : 0.0, ny = ll > 0.0 ? lx / ll : 1.0;
  const double *__restrict__ dk = k.discs;
#pragma clang loop unroll(disable)
  for (int q = 0; q < 2 * k.n; ++q) {
    const int m = q < k.n ? q : q - k.n;
    [[maybe_unused]] double cxm = 0.0, cym = 0.0;
    if constexpr (KMOV) { cxm = k.ctr[(size_t)(2 * m) * N + i]; cym = k.ctr[(size_t)(2 * m + 1) * N + i]; }
    const double R = dk[KMOV ? 2 * m : 3 * m + 2];
    if (!(R > 0.0)) continue;
    const double cx = KMOV ? cxm : dk[3 * m], cy = KMOV ? cym : dk[3 * m + 1], Rt = R * (1.0 + 1e-2);
    const double dx = x - cx, dy = y - cy, d2 = KMOV ? nlp_dot2(dx, dx, dy, dy) : dx * dx + dy * dy;
    if (KMOV ? fma(-R, R, d2) <= fma(Rt, Rt, -(R * R)) : d2 - R * R <= Rt * Rt - R * R) {
      const double dn = sqrt(d2);
      const bool deg = dn < 1e-12 * R;
      const double ux = deg ? nx : dx / dn, uy = deg ? ny : dy / dn;
      if constexpr (KMOV) { x = fma(Rt, ux, cx); y = fma(Rt, uy, cy); }
      else {
      x = cx + Rt * ux; y = cy + Rt * uy;
      }
    }
  }
}
// KEEP: what refuses a problem before its first store (wave-uniform): a disc with a non-finite entry, an end pose on or inside a disc,
// or a free node that the start rule leaves on or inside one (discs that cover the box, overlapping discs that leave no room).
__device__ __forceinline__ bool nlp_keep_bad(const NlpScen &s, const NlpKeepSet &k, const double *__restrict__ Wb, int N, int lane) {
  int bad = 0;
  const double *__restrict__ dk = k.discs;
#pragma clang loop unroll(disable)
  for (int m = 0; m < k.n; ++m) {
    const double cx = dk[3 * m], cy = dk[3 * m + 1], R = dk[3 * m + 2];
    bad |= !(fabs(cx) <= 1.79e308) || !(fabs(cy) <= 1.79e308) || !(fabs(R) <= 1.79e308);
    if (!(R > 0.0)) continue;
    const double ax = s.p0[0] - cx, ay = s.p0[1] - cy, bx = s.p1[0] - cx, by = s.p1[1] - cy;
    bad |= !(ax * ax + ay * ay - R * R > 0.0) || !(bx * bx + by * by - R * R > 0.0);
  }
  if (bad) return true;                      // (wave-uniform so far: the discs' table is)
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i < 1 || i >= N - 1) continue;
    double x = Wb[i], y = Wb[N + i];
    nlp_keep_start(s, k, x, y);
    x = nlp_box_push(x, s.lo[0], s.hi[0]); y = nlp_box_push(y, s.lo[1], s.hi[1]);
#pragma clang loop unroll(disable)
    for (int m = 0; m < k.n; ++m) {
      const double R = dk[3 * m + 2];
      if (!(R > 0.0)) continue;
      const double dx = x - dk[3 * m], dy = y - dk[3 * m + 1];
      bad |= !(dx * dx + dy * dy - R * R > 0.0);
    }
  }
  return __builtin_amdgcn_ballot_w64(bad != 0) != 0ull;
}
// KMOV: nlp_keep_bad for discs that move (the tracks and the start time are the caller's to check: nlp_mov_bad).  A radius that is not
// finite, an end pose on or inside a disc AT ITS OWN NODE'S TIME (the centres of node 0 and of node N - 1), or a free node that the
// start rule, taken with the node's own centres, leaves on or inside one.
__device__ __forceinline__ bool nlp_keep_bad(const NlpScen &s, const NlpKeepMovSet &k, const double *__restrict__ Wb, int N, int lane) {
  int bad = 0;
  const double *__restrict__ dk = k.discs;
#pragma clang loop unroll(disable)
  for (int m = 0; m < k.n; ++m) {
    const double *__restrict__ cxp = k.ctr + (size_t)(2 * m) * N, *__restrict__ cyp = cxp + N;
    const double ax = s.p0[0] - cxp[0], ay = s.p0[1] - cyp[0], bx = s.p1[0] - cxp[N - 1], by = s.p1[1] - cyp[N - 1];
    const double R = dk[2 * m];
    bad |= !(fabs(R) <= 1.79e308);
    if (!(R > 0.0)) continue;
    bad |= !(ax * ax + ay * ay - R * R > 0.0) || !(bx * bx + by * by - R * R > 0.0);
  }
  if (bad) return true;                      // (wave-uniform so far: the table and the two end centres are)
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i < 1 || i >= N - 1) continue;
    double x = Wb[i], y = Wb[N + i];
    nlp_keep_start<NLP_KMOV>(s, k, x, y, i, N);
    x = nlp_box_push(x, s.lo[0], s.hi[0]); y = nlp_box_push(y, s.lo[1], s.hi[1]);
#pragma clang loop unroll(disable)
    for (int m = 0; m < k.n; ++m) {
      const double cxm = k.ctr[(size_t)(2 * m) * N + i], cym = k.ctr[(size_t)(2 * m + 1) * N + i];
      const double R = dk[2 * m];
      if (!(R > 0.0)) continue;
      const double dx = x - cxm, dy = y - cym;
      bad |= !(nlp_keep_g(dx, dy, R) > 0.0);
    }
  }
  return __builtin_amdgcn_ballot_w64(bad != 0) != 0ull;
}
// FENCE: the start of a free node's position, behind the discs' rule where both are present (the caller has applied the box push, or
// nlp_keep_start has): every edge in index order, twice (at a corner a push off one edge can land in its neighbour's margin: the second
// pass undoes that) -- a node with g_k < kap_k moves along -a_k, the inward normal, to g_k = kap_k.  A node with g >= kap at every edge
// is not touched.  The caller re-applies the box push.
__device__ __forceinline__ void nlp_fence_start(const NlpFenceSet &f, double &x, double &y) {
#pragma clang loop unroll(disable)
  for (int q = 0; q < 2 * f.n; ++q) {
    const double *__restrict__ e = f.edges + 4 * (q < f.n ? q : q - f.n);
    if (!nlp_fence_present(e)) continue;
    const double gk = nlp_fence_g(e, x, y);
    if (gk < e[3]) {
      const double t = e[3] - gk;
      x = fma(-t, e[0], x); y = fma(-t, e[1], y);
    }
  }
}
// FENCE: what refuses a problem before its first store (wave-uniform): an edge with a non-finite entry, a present edge whose normal is
// off unit length by more than 1e-12 or whose kap is not positive, an end pose on or outside an edge, or a free node that the start
// rules -- the discs', then the edges', then the box push -- leave on or outside an edge or (KEEP) on or inside a disc.
template <unsigned F>
__device__ __forceinline__ bool nlp_fence_bad(const NlpScen &s, const NlpFenceProb &pb, const double *__restrict__ Wb, int N, int lane) {
  constexpr bool KEEP = NlpFeatures<F>::KEEP;
  int bad = 0;
  const NlpFenceSet &f = pb.fence;
#pragma clang loop unroll(disable)
  for (int k = 0; k < f.n; ++k) {
    const double *__restrict__ e = f.edges + 4 * k;
    bad |= !(fabs(e[0]) <= 1.79e308) || !(fabs(e[1]) <= 1.79e308) || !(fabs(e[2]) <= 1.79e308) || !(fabs(e[3]) <= 1.79e308);
    if (!nlp_fence_present(e)) continue;
    bad |= !(fabs(sqrt(nlp_dot2(e[0], e[0], e[1], e[1])) - 1.0) <= 1e-12) || !(e[3] > 0.0);
    bad |= !(nlp_fence_g(e, s.p0[0], s.p0[1]) > 0.0) || !(nlp_fence_g(e, s.p1[0], s.p1[1]) > 0.0);
  }
  if (bad) return true;                      // (wave-uniform so far: the edges' table is)
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i < 1 || i >= N - 1) continue;
    double x = Wb[i], y = Wb[N + i];
    if constexpr (KEEP) nlp_keep_start(s, pb.keep, x, y);
    else { x = nlp_box_push(x, s.lo[0], s.hi[0]); y = nlp_box_push(y, s.lo[1], s.hi[1]); }
    nlp_fence_start(f, x, y);
    x = nlp_box_push(x, s.lo[0], s.hi[0]); y = nlp_box_push(y, s.lo[1], s.hi[1]);
#pragma clang loop unroll(disable)
    for (int k = 0; k < f.n; ++k) {
      const double *__restrict__ e = f.edges + 4 * k;
      if (!nlp_fence_present(e)) continue;
      bad |= !(nlp_fence_g(e, x, y) > 0.0);
    }
    if constexpr (KEEP) {
      const double *__restrict__ dk = pb.keep.discs;
#pragma clang loop unroll(disable)
      for (int m = 0; m < pb.keep.n; ++m) {
        const double R = dk[3 * m + 2];
        if (!(R > 0.0)) continue;
        const double dx = x - dk[3 * m], dy = y - dk[3 * m + 1];
        bad |= !(dx * dx + dy * dy - R * R > 0.0);
      }
    }
  }
  return __builtin_amdgcn_ballot_w64(bad != 0) != 0ull;
}

// The solve of ONE problem by one wavefront (lane = threadIdx.x & 63): sc its scenario row, Wb [5][N] in/out, wsb its workspace,
// multb [3][N] or null, partner [2][N] frozen positions of the CostCollision partner or null.  Wave-uniform control flow.
// F: the feature set (NlpFeatures, at the head of the file); ex: the optional inputs that its members name (NlpExtra).
template <unsigned F = 0u>
__device__ __forceinline__ void nlp_solve_one(int N, double h, const d2d_nlp_opts &o, const double *__restrict__ sc, const double *partner,
                                              double *Wb, double *wsb, double *multb, int lane, NlpOut &out, unsigned long long *stamps, double *ldsw,
                                              const double *__restrict__ bnd, const NlpExtra &ex = NlpExtra{}) {
  NLP_FEATURES(F);
  const NlpModel md = ex.md;
  [[maybe_unused]] const NlpViaSet *via = ex.via;
  // diagnostics (D2D_NLP_STAMPS): cycles per phase -- merit, assembly, factorisation, back substitution, ratio tests, update
  unsigned long long st_t = 0, st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define NLP_STAMP(k) if (st_on) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[k] += t_ - st_t; st_t = t_; }
  const bool st_on = stamps != nullptr;
  if (st_on) st_t = __builtin_amdgcn_s_memtime();
  NlpScen s = nlp_load_scen(sc, o, bnd);
  if (sc[D2D_SC_BANKMAX] != 0.0) { s.sbank = s.skphi * (double)N; s.skphi = 0.0; }     // obj_scale * kbank (the row's S is obj_scale / N)
  NlpProbT<F> pb;
  if constexpr (FENCE) pb.fence = static_cast<const NlpKeepFenceSet *>(ex.keep)->fence;
  if constexpr (KEEP) pb.keep = *static_cast<const NlpKeepSetT<F & ~NLP_FENCE> *>(ex.keep);
  if constexpr (MOV) pb.mv = *ex.mv;
  if constexpr (VIA) pb.vm = via->vm;
  pb.N = N; pb.h = h;
  pb.W = Wb;
  pb.ws = wsb;
  pb.mu = multb ? multb : pb.ws + (size_t)WS_MU * N;
  pb.partner = partner;
  pb.pmask = ex.pmask;
  pb.lds = ldsw;
  pb.wf = ex.wf; pb.t0 = ex.t_start;
  // (a row whose bounds are unset or inverted would give a zero-width box, infinite duals and NaN pivots for
  // outer_max x 30 assemblies -- refuse it at once)
  {
    bool bad = !(s.hi[3] > s.lo[3]) || !(s.hi[4] > s.lo[4]) || !(s.lo[4] > 0.0) || !(s.hi[0] > s.lo[0]) || !(s.hi[1] > s.lo[1]) || !(s.hi[2] > s.lo[2]);
    for (int c = 0; c < 3; ++c) bad = bad || !(fabs(s.p0[c]) <= 1.79e308) || !(fabs(s.p1[c]) <= 1.79e308);
    if constexpr (MODEL) {            // a model with a non-finite entry is refused like a bad row
      int nf = 0;
      for (int i = lane; i < N; i += 64) {
#pragma unroll
        for (int c = 0; c < NLP_NV; ++c) nf |= !(fabs(md.g[c * N + i]) <= 1.79e308) || !(fabs(md.Wc[c * N + i]) <= 1.79e308);
#pragma unroll
        for (int k = 0; k < 15; ++k) nf |= !(fabs(md.H[k * N + i]) <= 1.79e308);
      }
      bad = bad || __builtin_amdgcn_ballot_w64(nf != 0) != 0ull;
    }
    if constexpr (FREE) {             // the box of h: 0 < h_lo < h_hi, k_dur >= 0, a start that is 0 (the launch's h) or finite
      const double hl = ex.free_row[0], hh = ex.free_row[1], kd = ex.free_row[2], hs = ex.free_row[3];
      bad = bad || !(hl > 0.0) || !(hl < hh) || !(hh <= 1.79e308) || !(kd >= 0.0) || !(kd <= 1.79e308) || !(fabs(hs) <= 1.79e308);
      if (lane == 0) *ex.h_out = __builtin_nan("");
    }
    if constexpr (KEEP) bad = bad || nlp_keep_bad(s, pb.keep, Wb, N, lane);
    if constexpr (FENCE) bad = bad || nlp_fence_bad<F>(s, pb, Wb, N, lane);
    if (bad) {
      out.cost = out.feas = __builtin_nan(""); out.iters = 0; out.status = D2D_ST_NONFINITE;
      return;
    }
  }
  // ---- start: end conditions in place, everything else pushed strictly inside the box; duals on the central path
  double mub = o.mub0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    if (i >= N) continue;
    [[maybe_unused]] int vmi = 0;
    [[maybe_unused]] double pin[3] = {0.0, 0.0, 0.0};
    if constexpr (VIA) {                     // the node's fixed set and pinned values: the table's rows that name it (wave-uniform loads)
      if (i == 0 || i == N - 1) vmi = 7;
#pragma clang loop unroll(disable)
      for (int e = 0; e < via->n; ++e) {
        const double *__restrict__ p = via->pts + 5 * e;
        const int m = (int)p[1];
        if (m == 0 || (int)p[0] != i) continue;
        vmi |= m;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if ((m >> c) & 1) pin[c] = p[2 + c];
      }
      via->vm[i] = vmi;
    }
    [[maybe_unused]] double kxy[2] = {0.0, 0.0};
    if constexpr (KEEP) {
      kxy[0] = NLP_W(0, i); kxy[1] = NLP_W(1, i);
      nlp_keep_start<F>(s, pb.keep, kxy[0], kxy[1], i, N);
    }
    if constexpr (FENCE) {
      if constexpr (!KEEP) { kxy[0] = nlp_box_push(NLP_W(0, i), s.lo[0], s.hi[0]); kxy[1] = nlp_box_push(NLP_W(1, i), s.lo[1], s.hi[1]); }
      nlp_fence_start(pb.fence, kxy[0], kxy[1]);
    }
#pragma unroll
    for (int c = 0; c < NLP_NV; ++c) {
      double w = NLP_W(c, i);
      if constexpr (KEEP || FENCE) { if (c < 2) w = kxy[c]; }
      double zl = 0.0, zu = 0.0;
      if (nlp_fixed_at<F>(i, N, c, vmi)) {
        if constexpr (VIA) w = (i == 0) ? s.p0[c] : (i == N - 1 ? s.p1[c] : pin[c]);
        else
        w = (i == 0) ? s.p0[c] : s.p1[c];
      } else {
        const bool hl = s.lo[c] > -1e299, hu = s.hi[c] < 1e299;
        const double width = (hl && hu) ? s.hi[c] - s.lo[c] : 1e300;
        const double kap = fmin(1e-2 * fmax(1.0, fabs(w)), 1e-2 * width);
        if (hl) w = fmax(w, s.lo[c] + kap);
        if (hu) w = fmin(w, s.hi[c] - kap);
        if (hl) zl = mub / (w - s.lo[c]);
        if (hu) zu = mub / (s.hi[c] - w);
      }
      NLP_W(c, i) = w;
      if constexpr (KEEP || FENCE) { if (c < 2) kxy[c] = w; }
      NLP_P(WS_ZL + c, i) = zl; NLP_P(WS_ZU + c, i) = zu;
      NLP_DW(c, i) = 0.0;
    }
    if constexpr (KEEP) {                    // the discs' duals on the central path; 0 at the end nodes and for absent discs
      const double *__restrict__ dk = pb.keep.discs;
#pragma clang loop unroll(disable)
      for (int m = 0; m < pb.keep.n; ++m) {
        [[maybe_unused]] double cxm = 0.0, cym = 0.0;
        if constexpr (KMOV) { cxm = pb.keep.ctr[(size_t)(2 * m) * N + i]; cym = pb.keep.ctr[(size_t)(2 * m + 1) * N + i]; }
        const double R = dk[KMOV ? 2 * m : 3 * m + 2], dx = kxy[0] - (KMOV ? cxm : dk[3 * m]), dy = kxy[1] - (KMOV ? cym : dk[3 * m + 1]);
        // (KMOV: the static kernels fuse the OTHER product in this one place)
        pb.keep.z[(size_t)m * N + i] = (R > 0.0 && i >= 1 && i < N - 1) ? mub / (KMOV ? nlp_keep_g(dy, dx, R) : dx * dx + dy * dy - R * R) : 0.0;
      }
    }
    if constexpr (FENCE) {                   // the edges' duals on the central path; 0 at the end nodes and for absent edges
#pragma clang loop unroll(disable)
      for (int k = 0; k < pb.fence.n; ++k) {
        const double *__restrict__ e = pb.fence.edges + 4 * k;
        pb.fence.z[(size_t)k * N + i] = (nlp_fence_present(e) && i >= 1 && i < N - 1) ? mub / nlp_fence_g(e, kxy[0], kxy[1]) : 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) NLP_MU(k, i) = 0.0;
  }
  [[maybe_unused]] double du = 0.0, ut = 0.0;          // FREE: the step of u, and the value of u that nlp_merit reads the equalities at
  if constexpr (FREE) {                      // u = 1 / h pushed strictly inside its box like a node variable, its duals on the central path
    const double hs = ex.free_row[3] != 0.0 ? ex.free_row[3] : h;
    pb.ulo = 1.0 / ex.free_row[1]; pb.uhi = 1.0 / ex.free_row[0]; pb.kd = ex.free_row[2] * (double)(N - 1);
    double u = 1.0 / hs;
    const double kap = fmin(1e-2 * fmax(1.0, fabs(u)), 1e-2 * (pb.uhi - pb.ulo));
    u = fmin(fmax(u, pb.ulo + kap), pb.uhi - kap);
    pb.u = u; pb.h = 1.0 / u;
    pb.zul = mub / (u - pb.ulo); pb.zuu = mub / (pb.uhi - u);
  }
  nlp_phase_sync();
  const bool rec_lds = !FREE && !o.serial && N <= NLP_BCR_LDS_NODES;       // the reduced records go from the assembly to the cyclic reduction through the LDS
  double rho = o.rho0, lam = D2D_LM_LAMBDA0, feas_prev = INFINITY;
  int total_inner = 0, status = D2D_ST_MAXITER;
  double err = 0.0, cost_ref = 0.0, feas = 0.0;
  int n_stalled = 0;                        // outer iterations in a row at the largest penalty without feasibility progress
  // CostBank max mode ends "converged in value": a whole batch of steps that no longer lowers the merit function.  That test needs
  // a window of its own length, whatever the batch of the schedule is: D2D_NLP_BANKMAX_BATCHES batches in one (same step budget).
  const int inner_n = s.sbank > 0.0 ? D2D_NLP_BANKMAX_BATCHES * o.inner_max : o.inner_max;
  const int outer_n = s.sbank > 0.0 ? (o.outer_max + D2D_NLP_BANKMAX_BATCHES - 1) / D2D_NLP_BANKMAX_BATCHES : o.outer_max;
  for (int outer = 1; outer <= outer_n; ++outer) {
    const double tol_in = fmax(fmax(o.opt_tol, fmin(1e-1, 10.0 * mub)), D2D_NLP_GRAD_FLOOR * rho);
    // merit value of the current point for this (mub, rho, mu): one pass here, afterwards the accepted trial's value
    NLP_STAMP(7)
    double phi0;
    if constexpr (FREE) ut = pb.u;
    phi0 = nlp_merit<F>(pb, s, sc, lane, 0.0, rho, mub, nullptr, nullptr, md, ut);
    const double phi_first = phi0;
    NLP_STAMP(0)
    bool accepted = false;
    for (int it = 0; it < inner_n; ++it) {
      ++total_inner;
      bool converged = false;
      accepted = false;
      const int imax = s.sbank > 0.0 ? nlp_bank_argmax(pb, lane) : -1;
      for (int tr = 0; tr < 30; ++tr) {
        bool pd;
        [[maybe_unused]] double ru = 0.0, dfull = 0.0;
        if constexpr (FREE) {
          NlpFreeRow fr;
          err = nlp_assemble<F>(pb, s, sc, lane, rho, mub, lam, &pd, imax, false, md, &fr);
          // the row of u: half gradient, KKT error, right-hand side, damped half curvature
          const double u = pb.u, sl = u - pb.ulo, su = pb.uhi - u;
          const double g_u = -0.5 * pb.kd / (u * u) + fr.gu;
          err = fmax(fmax(err, fabs(2.0 * g_u - pb.zul + pb.zuu)), fmax(fabs(pb.zul * sl - mub), fabs(pb.zuu * su - mub)));
          ru = -(2.0 * g_u - mub / sl + mub / su);
          const double d0 = pb.kd / (u * u * u) + fr.dd + 0.5 * (pb.zul / sl + pb.zuu / su);
          dfull = d0 + lam * fmax(fabs(d0), 1e-12);
        } else
        err = nlp_assemble<F>(pb, s, sc, lane, rho, mub, lam, &pd, imax, rec_lds, md);  // (a retry with another damping assembles again: rare)
        nlp_phase_sync();
        NLP_STAMP(1)
        if (tr == 0 && err <= tol_in) { converged = true; break; }
        if constexpr (FREE) {                // two passes of the cyclic reduction: right-hand side, then border (each loads its own records)
          if (pd) pd = nlp_bcr(pb.ws + (size_t)WS_SIN * N, pb.ws + (size_t)WS_SF * N, pb.ws + (size_t)WS_DS * N, pb.lds, N, false);
          if (pd) {
            nlp_phase_sync();
            pd = nlp_bcr(pb.ws + (size_t)WSF_SIN2 * N, pb.ws + (size_t)WS_SF * N, pb.ws + (size_t)WSF_DS2 * N, pb.lds, N, false);
          }
        } else
        if (pd) {
          if (o.serial) pd = nlp_factor(pb.ws + (size_t)WS_SIN * N, pb.ws + (size_t)WS_SF * N, pb.ws + (size_t)WS_UP * N, N);   // (UP is free by now)
          else pd = nlp_bcr(pb.ws + (size_t)WS_SIN * N, pb.ws + (size_t)WS_SF * N, pb.ws + (size_t)WS_DS * N, pb.lds, N, rec_lds);
        }
        NLP_STAMP(2)
        if (!pd) { lam = fmin(lam * 8.0, D2D_LM_LAMBDA_MAX); continue; }
        nlp_phase_sync();
        if constexpr (VIA) { if (o.serial) nlp_backsolve<true>(pb.ws + (size_t)WS_SF * N, pb.ws + (size_t)WS_UP * N, pb.ws + (size_t)WS_DS * N, N, pb.vm); }
        else
        if (o.serial) nlp_backsolve(pb.ws + (size_t)WS_SF * N, pb.ws + (size_t)WS_UP * N, pb.ws + (size_t)WS_DS * N, N);
        nlp_phase_sync();
        NLP_STAMP(3)
        const double tau = fmax(0.99, 1.0 - mub);
        double dphi, amax, az;
        if constexpr (FREE) {
          const bool spd = nlp_recover_free<F>(pb, s, lane, mub, tau, ru, dfull, &dphi, &amax, &az, &du);
          nlp_phase_sync();
          NLP_STAMP(4)
          if (!spd) { lam = fmin(lam * 8.0, D2D_LM_LAMBDA_MAX); continue; }
        } else {
        nlp_recover_stats<F>(pb, s, lane, mub, tau, &dphi, &amax, &az);
        nlp_phase_sync();
        NLP_STAMP(4)
        }
        if (!(dphi < 0.0)) { lam = fmin(lam * 8.0, D2D_LM_LAMBDA_MAX); continue; }
        double a = amax, pt = 0.0;
        bool ok = false;
        for (int ls = 0; ls < 8; ++ls) {
          if constexpr (FREE) ut = pb.u + a * du;
          pt = nlp_merit<F>(pb, s, sc, lane, a, rho, mub, nullptr, nullptr, md, ut);
          if (pt <= phi0 + 1e-4 * a * dphi) { ok = true; break; }
          a *= 0.5;
        }
        NLP_STAMP(0)
        if (ok) {
          phi0 = pt;
          nlp_apply<F>(pb, s, lane, a, az, mub);
          if constexpr (FREE) {              // u and its duals move like a node variable (nlp_apply)
            const double u = pb.u, un = u + a * du, sl = u - pb.ulo, su = pb.uhi - u;
            const double ml = mub / (un - pb.ulo), mh = mub / (pb.uhi - un);
            pb.zul = fmin(fmax(pb.zul + az * ((mub - pb.zul * du) / sl - pb.zul), 1e-10 * ml), 1e10 * ml);
            pb.zuu = fmin(fmax(pb.zuu + az * ((mub + pb.zuu * du) / su - pb.zuu), 1e-10 * mh), 1e10 * mh);
            pb.u = un; pb.h = 1.0 / un;
          }
          nlp_phase_sync();
          NLP_STAMP(5)
          if (a == amax) lam = fmax(lam / 3.0, D2D_LM_LAMBDA_MIN);
          accepted = true;
          break;
        }
        lam = fmin(lam * 4.0, D2D_LM_LAMBDA_MAX);
      }
      if (converged || !accepted) break;
    }
    if constexpr (FREE) ut = pb.u;
    (void)nlp_merit<F>(pb, s, sc, lane, 0.0, rho, mub, &cost_ref, &feas, md, ut);
    if (!(fabs(phi0) <= 1.79e308) || !(fabs(err) <= 1.79e308)) { status = D2D_ST_NONFINITE; break; }
    if (feas <= o.feas_tol && mub <= o.mub_min * 1.0001 && err <= tol_in) { status = D2D_ST_CONVERGED; break; }
    // CostBank max mode: the one-hot cost_grad has no zero where two nodes share the maximum (they do at a min-max optimum): the
    // solve ends converged IN VALUE -- feasible, barrier at its floor, a whole batch of steps that lowered the merit by no more
    // than D2D_NLP_BANKMAX_VALUE_TOL of itself (oracle/nlp.py solve)
    if (s.sbank > 0.0 && feas <= o.feas_tol && mub <= o.mub_min * 1.0001 && (phi_first - phi0) <= D2D_NLP_BANKMAX_VALUE_TOL * (1.0 + fabs(phi0))) {
      status = D2D_ST_CONVERGED; break;
    }
    // the inner problem is not solved yet and the batch still lowered the merit function by more than rounding: same multipliers,
    // penalty and barrier parameter, another batch of steps -- the schedule must not run ahead of the iterate
    if (err > tol_in && accepted && (phi_first - phi0) > (s.sbank > 0.0 ? D2D_NLP_BANKMAX_VALUE_TOL : D2D_NLP_GATE_PROGRESS) * (1.0 + fabs(phi0))) continue;
    // an infeasible problem (e.g. end points too far apart for v_max) or an infeasible stationary point of the violation: the
    // penalty grows tenfold per solved inner problem and the violation no longer halves -- give up instead of running
    // outer_max x inner_max steps
    n_stalled = (feas > 0.5 * feas_prev && feas > 1e3 * o.feas_tol) ? n_stalled + 1 : 0;
    if (n_stalled >= (rho >= D2D_NLP_RHO_MAX ? 3 : D2D_NLP_STALL_OUTERS)) { status = D2D_ST_STALLED; break; }
    // first-order multiplier update (lambda = 2 rho mu); the penalty grows when feasibility stalls
    const bool grow = feas > 0.25 * feas_prev && rho < D2D_NLP_RHO_MAX;
    for (int i0 = 0; i0 < N; i0 += 64) {
      const int i = i0 + lane;
      if (i < 1 || i >= N) continue;
      double wp[3], w[NLP_NV], c3[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) wp[c] = NLP_W(c, i - 1);
#pragma unroll
      for (int c = 0; c < NLP_NV; ++c) w[c] = NLP_W(c, i);
      if constexpr (FREE) nlp_constraint(s, pb.h, wp, w, c3);
      else
      nlp_constraint<WIND>(s, h, wp, w, c3, pb.wf, NLP_T(i));
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double m = NLP_MU(k, i) + c3[k];
        NLP_MU(k, i) = grow ? m / D2D_NLP_RHO_GROW : m;
      }
    }
    nlp_phase_sync();
    if (grow) rho *= D2D_NLP_RHO_GROW;
    feas_prev = feas;
    mub = fmax(o.mub_min, fmin(0.2 * mub, mub * sqrt(mub)));
  }
  if constexpr (FREE) ut = pb.u;
  (void)nlp_merit<F>(pb, s, sc, lane, 0.0, rho, mub, &cost_ref, &feas, md, ut);
  if constexpr (FREE) { if (lane == 0) *ex.h_out = pb.h; }
  out.cost = cost_ref; out.feas = feas; out.iters = total_inner; out.status = status;
  if (lane == 0 && st_on) {
    NLP_STAMP(7)
    for (int k = 0; k < 8; ++k) stamps[k] = st_acc[k];
    stamps[8] = (unsigned long long)total_inner;
  }
#undef NLP_STAMP
}

#ifndef NLP_WAVES_PER_SIMD
#define NLP_WAVES_PER_SIMD 2       // (A/B: -DNLP_WAVES_PER_SIMD=1 gives the assembly 512 registers and no scratch)
#endif
#ifndef NLP_WIND_WAVES_PER_SIMD
#define NLP_WIND_WAVES_PER_SIMD 2
#endif

// the next ticket of the hand-out queue: lane 0 draws it, the wavefront reads it
__device__ __forceinline__ int nlp_next_ticket(int32_t *queue, int lane) {
  int tn = 0;
  if (lane == 0) tn = (int)gridDim.x + atomicAdd(queue, 1);
  return __builtin_amdgcn_readfirstlane(tn);
}

// One wavefront per problem.  Node-parallel phases (merit, assembly, step statistics, update) run with lane = node; the two
// block recursions are serial in the nodes and run wave-uniform.  Control flow is uniform: no lane waits for another problem.
// Two waves per SIMD: the assembly spills for it (640-708 B / lane, once per Newton step; the serial recursions are separate functions
// and do not).  Round 2 measured +12 % problems/s for it; since round 4's schedule change, and again after round 5's, one
// wave per SIMD (-DNLP_WAVES_PER_SIMD=1: no spill in the kernel) runs at the SAME speed at 512, 4096 and 65 536 problems -- the
// spills are off the critical path, and so is the second wave.
// Persistent: the grid is one wavefront per wave slot of the chip (or per problem, if there are fewer), problems are handed out through
// a device counter, and the WORKSPACE BELONGS TO THE SLOT (work + blockIdx.x * WS_TOTAL * N), not to the problem: nothing in it
// outlives a solve, and with one workspace per problem every solve streamed its 100+ kB through cold lines while the ones it
// followed were written back -- slots keep the chip's working set at (resident waves) x (workspace) whatever the batch.
// The hand-out loop stands here once more, not in nlp_handout_body, which the wind and via kernels share: built through
// such a __forceinline__ body (tried with and without __restrict__ on its parameters, and with the ticket in the for-increment) this
// kernel kept 255 VGPRs and 672 B / lane of scratch but its spills moved (SGPR 206 -> 204 .. 216, VGPR 122 -> 124) and 4300 - 5600 of
// its 12 223 lines of ISA with them.  The benchmark times this kernel, so it keeps its code; only the ticket is shared.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WAVES_PER_SIMD, NLP_WAVES_PER_SIMD)))
nlp_solve_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, const double *partner, double *W,
                 double *work, double *mult, double *__restrict__ cost_out, double *__restrict__ feas_out,
                 int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out, unsigned long long *stamps, int32_t *queue) {
  const int lane = threadIdx.x;
  extern __shared__ __attribute__((aligned(16))) double nlp_lds[];
  double *wsb = work + (size_t)blockIdx.x * WS_TOTAL * N;
  const int32_t *__restrict__ order = o.order;
  for (int t = blockIdx.x; t < B;) {
    const int b = order ? __builtin_amdgcn_readfirstlane(order[t]) : t;
    if ((unsigned)b >= (unsigned)B) {        // (an entry that is no problem index is skipped, not dereferenced)
      t = nlp_next_ticket(queue, lane);
      continue;
    }
    NlpOut out;
    nlp_solve_one(N, h, o, scen + (size_t)b * D2D_SCEN_STRIDE, partner ? partner + (size_t)b * 2 * N : nullptr, W + (size_t)b * NLP_NV * N,
                  wsb, mult ? mult + (size_t)b * 3 * N : nullptr, lane, out, b == 0 ? stamps : nullptr, nlp_lds,
                  o.bounds ? o.bounds + (size_t)b * 4 : nullptr);
    if (lane == 0) {
      cost_out[b] = out.cost;
      feas_out[b] = out.feas;
      if (iters_out) iters_out[b] = out.iters;
      if (status_out) status_out[b] = out.status;
    }
    nlp_phase_sync();                        // (the next problem's first stores to the workspace follow this one's last loads)
    t = nlp_next_ticket(queue, lane);
  }
}

// d2d_mov_sample: the centres of the moving discs at the node times, ctr [G][n_mov][2][N].  A workgroup per (problem or scenario,
// disc), lane = node; the track's knots are a table of at most D2D_MOV_MAX_KNOT rows that every lane walks (scalar loads).  The
// centre is linear between the two knots that bracket t = t_start[g] + i h (one multiply-add, not accumulated) and held at the first
// or last knot outside them; at a segment's end it is that knot exactly, so knots repeated behind the last one change nothing.
// Tracks are not validated here (the solve kernels do that): whatever the knots hold, no index leaves the track.
__global__ void __launch_bounds__(64)
nlp_mov_sample_kernel(int N, double h, const double *__restrict__ t_start, d2d_moving_obstacles mv, double *__restrict__ ctr) {
  const int g = blockIdx.x / mv.n_mov;
  const double *__restrict__ kn = mv.knots + (size_t)blockIdx.x * mv.n_knot * 3;
  double *__restrict__ out = ctr + (size_t)blockIdx.x * 2 * N;
  const double t0 = t_start[g];
  for (int i = threadIdx.x; i < N; i += 64) {
    const double t = t0 + (double)i * h;
    int k = 0;                               // the segment [knot k, knot k + 1] that holds t, the first or last one outside the knots
    for (int q = 1; q < mv.n_knot - 1; ++q)
      if (kn[3 * q] <= t) k = q;
    const double ta = kn[3 * k], xa = kn[3 * k + 1], ya = kn[3 * k + 2], tb = kn[3 * k + 3], xb = kn[3 * k + 4], yb = kn[3 * k + 5];
    const double u = fmax((t - ta) / (tb - ta), 0.0);
    out[i] = u >= 1.0 ? xb : fma(u, xb - xa, xa);
    out[N + i] = u >= 1.0 ? yb : fma(u, yb - ya, ya);
  }
}

// The tracks of problem or scenario g, checked by every wavefront that solves against them before its first solve: a non-finite knot,
// times that do not increase strictly, or a kind that is neither 0 nor 1.  Wave-uniform.
__device__ __forceinline__ bool nlp_mov_bad(const d2d_moving_obstacles &mv, int g, int lane) {
  int bad = 0;
  const double *__restrict__ kn = mv.knots + (size_t)g * mv.n_mov * mv.n_knot * 3;
  for (int e = lane; e < mv.n_mov * mv.n_knot; e += 64) {
    const double t = kn[3 * e];
    bad |= !(fabs(t) <= 1.79e308) || !(fabs(kn[3 * e + 1]) <= 1.79e308) || !(fabs(kn[3 * e + 2]) <= 1.79e308);
    if (e % mv.n_knot != 0) bad |= !(t > kn[3 * (e - 1)]);
  }
  for (int m = lane; m < mv.n_mov; m += 64) {
    const double kind = mv.disc[((size_t)g * mv.n_mov + m) * 2 + 1];
    bad |= !(kind == 0.0 || kind == 1.0);
  }
  return __builtin_amdgcn_ballot_w64(bad != 0) != 0ull;
}

// The hand-out loop's report of one problem: the single-problem twin of nlp_groups_report.
__device__ __forceinline__ void nlp_report(int b, int lane, const NlpOut &out, double *cost_out, double *feas_out, int32_t *iters_out,
                                           int32_t *status_out) {
  if (lane == 0) {
    cost_out[b] = out.cost;
    feas_out[b] = out.feas;
    if (iters_out) iters_out[b] = out.iters;
    if (status_out) status_out[b] = out.status;
  }
}

// nlp_solve_kernel's persistent hand-out around the other instantiations of the solve (no partner): one body for the hand-out kernels
// below, switched at compile time by F.  The field is shared by the batch and travels as a kernel argument (scalar registers); its
// control points are a small table that every wavefront reads and that stays in L2.  What the members of F read HERE, per problem:
// T_AT: t_at [B], read when the equalities or a track need it; a problem whose start time is not finite is refused before its solve.
//   Else the start time is the scalar t_start of d2d_nlp_solve_wind, which the host has checked.
// MOV: the centre planes ctr [B][n_mov][2][N], sampled ahead of this launch; a problem whose tracks are unusable is refused (n_mov = 0:
//   nothing moves).  VIA: via->pts [B][n_via][5] and the plane of the nodes' fixed sets vwork [B][N]; unusable pins refuse it likewise.
// FREE: free_rows [B][4] and h_out [B]; the slot's workspace has the planes of the border behind the others (WSF_TOTAL); stamps.
// KEEP: keep->discs [B][n_keep][3] and the planes of their duals kwork [B][n_keep][N] (the problem's, not the slot's: a result).  KMOV:
//   the hard discs in mv and ctr, tracks checked like MOV's, kwork [B][n_mov][N].  FENCE: fence->edges [B][n_edge][4] and fwork
//   [B][n_edge][N] beside the discs' (n_keep may be 0: keep->discs and kwork are then not read).
// A refused problem's W is not touched.  The pointer parameters carry no __restrict__ (the kernels' do), as in nlp_groups_body.
template <unsigned F>
__device__ __forceinline__ void nlp_handout_body(int B, int N, double h, const d2d_nlp_opts &o, const double *scen, double *W, double *work,
                                                 double *mult, double *cost_out, double *feas_out, int32_t *iters_out, int32_t *status_out,
                                                 int32_t *queue, const d2d_wind_field *wf, double t_start, const double *t_at = nullptr,
                                                 const d2d_moving_obstacles *mv = nullptr, const double *ctr = nullptr, const d2d_via_points *via = nullptr,
                                                 int32_t *vwork = nullptr, const double *free_rows = nullptr, double *h_out = nullptr,
                                                 [[maybe_unused]] unsigned long long *stamps = nullptr, [[maybe_unused]] const d2d_keep_out *keep = nullptr,
                                                 [[maybe_unused]] double *kwork = nullptr, [[maybe_unused]] const d2d_fence *fence = nullptr,
                                                 [[maybe_unused]] double *fwork = nullptr) {
  NLP_FEATURES(F);
  static_assert(!(MODEL || PAIRS), "the hand-out loop solves single problems under the structured objective");
  const int lane = threadIdx.x;
  extern __shared__ __attribute__((aligned(16))) double nlp_lds[];
  double *wsb = work + (size_t)blockIdx.x * (FREE ? WSF_TOTAL : WS_TOTAL) * N;
  const int32_t *__restrict__ order = o.order;
  for (int t = blockIdx.x; t < B;) {
    const int b = order ? __builtin_amdgcn_readfirstlane(order[t]) : t;
    if ((unsigned)b >= (unsigned)B) {        // (an entry that is no problem index is skipped, not dereferenced)
      t = nlp_next_ticket(queue, lane);
      continue;
    }
    NlpOut out;
    double t0 = t_start;
    bool bad = false;
    if constexpr (T_AT) {
      t0 = 0.0;
      if (WIND || ((MOV || KMOV) && mv->n_mov > 0)) {
        t0 = nlp_first_lane(t_at[b]);
        bad = !(fabs(t0) <= 1.79e308);
      }
    }
    [[maybe_unused]] NlpMovSet ms{nullptr, nullptr, 0};
    if constexpr (MOV || KMOV) {
      if (mv->n_mov > 0) bad = bad || nlp_mov_bad(*mv, b, lane);
    }
    if constexpr (MOV) ms = NlpMovSet{ctr + (size_t)b * mv->n_mov * 2 * N, mv->disc + (size_t)b * mv->n_mov * 2, mv->n_mov};
    const double *sc = scen + (size_t)b * D2D_SCEN_STRIDE, *bnd = o.bounds ? o.bounds + (size_t)b * 4 : nullptr;
    [[maybe_unused]] NlpViaSet vs{nullptr, nullptr, 0};
    if constexpr (VIA) {
      vs = NlpViaSet{via->pts + (size_t)b * via->n_via * 5, vwork + (size_t)b * N, via->n_via};
      bad = bad || nlp_via_bad(vs.pts, vs.n, N, sc, o, bnd, lane);
    }
    if (bad) {
      out.cost = out.feas = __builtin_nan(""); out.iters = 0; out.status = D2D_ST_NONFINITE;
    } else if constexpr (FREE && FENCE) {    // the free step inside both families: the sets of the common call below, the row of the one that follows
      NlpKeepFenceSet ks{};
      static_cast<NlpKeepSet &>(ks) = NlpKeepSet{keep->discs + (size_t)b * keep->n_keep * 3, kwork + (size_t)b * keep->n_keep * N, keep->n_keep};
      ks.fence = NlpFenceSet{fence->edges + (size_t)b * fence->n_edge * 4, fwork + (size_t)b * fence->n_edge * N, fence->n_edge};
      nlp_solve_one<F>(N, h, o, sc, nullptr, W + (size_t)b * NLP_NV * N, wsb, mult ? mult + (size_t)b * 3 * N : nullptr, lane, out, nullptr, nlp_lds, bnd,
                       NlpExtra{{nullptr, nullptr, nullptr}, nullptr, 0.0, 0u, nullptr, nullptr, free_rows + (size_t)b * 4, h_out + b, &ks});
    } else if constexpr (FREE) {             // (a call of its own: through the one below, this kernel's refusal block came out reordered -- DESIGN 5.28)
      nlp_solve_one<NLP_FREE>(N, h, o, sc, nullptr, W + (size_t)b * NLP_NV * N, wsb, mult ? mult + (size_t)b * 3 * N : nullptr, lane, out,
                              b == 0 ? stamps : nullptr, nlp_lds, bnd,
                              NlpExtra{{nullptr, nullptr, nullptr}, nullptr, 0.0, 0u, nullptr, nullptr, free_rows + (size_t)b * 4, h_out + b});
    } else {
      [[maybe_unused]] NlpKeepSetT<F> ks{};  // (filled member by member: assigned from a braced NlpKeepMovSet the KMOV kernels spilled two more scalars)
      if constexpr (KMOV) { ks.discs = mv->disc + (size_t)b * mv->n_mov * 2; ks.z = kwork + (size_t)b * mv->n_mov * N; ks.n = mv->n_mov; ks.ctr = ctr + (size_t)b * mv->n_mov * 2 * N; }
      else if constexpr (KEEP) static_cast<NlpKeepSet &>(ks) = NlpKeepSet{keep->discs + (size_t)b * keep->n_keep * 3, kwork + (size_t)b * keep->n_keep * N, keep->n_keep};
      if constexpr (FENCE) ks.fence = NlpFenceSet{fence->edges + (size_t)b * fence->n_edge * 4, fwork + (size_t)b * fence->n_edge * N, fence->n_edge};
      nlp_solve_one<F & ~NLP_T_AT>(N, h, o, sc, nullptr, W + (size_t)b * NLP_NV * N, wsb, mult ? mult + (size_t)b * 3 * N : nullptr, lane, out, nullptr, nlp_lds,
                                   bnd, NlpExtra{{nullptr, nullptr, nullptr}, wf, t0, 0u, &ms, &vs, nullptr, nullptr, KEEP ? &ks : nullptr});
    }
    nlp_report(b, lane, out, cost_out, feas_out, iters_out, status_out);
    nlp_phase_sync();                        // (the next problem's first stores to the workspace follow this one's last loads)
    t = nlp_next_ticket(queue, lane);
  }
}

// d2d_nlp_solve_wind: the field and one start time for the batch, a host scalar
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WIND_WAVES_PER_SIMD, NLP_WIND_WAVES_PER_SIMD)))
nlp_solve_wind_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, double *W, double *work, double *mult,
                      double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                      int32_t *__restrict__ status_out, int32_t *queue, d2d_wind_field wf, double t_start) {
  nlp_handout_body<NLP_WIND>(B, N, h, o, scen, W, work, mult, cost_out, feas_out, iters_out, status_out, queue, &wf, t_start);
}

// d2d_nlp_solve_free: every problem with its own free time step (constant wind, static discs, no partner)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WIND_WAVES_PER_SIMD, NLP_WIND_WAVES_PER_SIMD)))
nlp_solve_free_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, double *W, double *work, double *mult,
                      double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                      int32_t *__restrict__ status_out, int32_t *queue, const double *__restrict__ free_rows, double *__restrict__ h_out,
                      unsigned long long *stamps) {
  nlp_handout_body<NLP_FREE>(B, N, h, o, scen, W, work, mult, cost_out, feas_out, iters_out, status_out, queue, nullptr, 0.0, nullptr, nullptr,
                             nullptr, nullptr, nullptr, free_rows, h_out, stamps);
}

// d2d_nlp_solve_free_fence: the free time step outside every problem's static hard discs and inside its convex polygon (constant wind)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WIND_WAVES_PER_SIMD, NLP_WIND_WAVES_PER_SIMD)))
nlp_solve_free_fence_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, double *W, double *work, double *mult,
                            double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                            int32_t *__restrict__ status_out, int32_t *queue, const double *__restrict__ free_rows, double *__restrict__ h_out,
                            d2d_keep_out keep, double *kwork, d2d_fence fence, double *fwork) {
  nlp_handout_body<NLP_FREE | NLP_KEEP | NLP_FENCE>(B, N, h, o, scen, W, work, mult, cost_out, feas_out, iters_out, status_out, queue, nullptr, 0.0,
                                                    nullptr, nullptr, nullptr, nullptr, nullptr, free_rows, h_out, nullptr, &keep, kwork, &fence, fwork);
}

// d2d_nlp_solve_keepout: outside every problem's hard discs -- the rows' constant wind or the field (WIND), the start time per problem
template <bool WIND>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WIND_WAVES_PER_SIMD, NLP_WIND_WAVES_PER_SIMD)))
nlp_solve_keepout_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, double *W, double *work, double *mult,
                         double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                         int32_t *__restrict__ status_out, int32_t *queue, d2d_wind_field wf, const double *__restrict__ t_start,
                         d2d_keep_out keep, double *kwork) {
  nlp_handout_body<NLP_WIND * WIND | NLP_T_AT | NLP_KEEP>(B, N, h, o, scen, W, work, mult, cost_out, feas_out, iters_out, status_out, queue, &wf, 0.0,
                                                          t_start, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &keep, kwork);
}

// d2d_nlp_solve_fence: inside every problem's convex polygon and outside its hard discs
template <bool WIND>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WIND_WAVES_PER_SIMD, NLP_WIND_WAVES_PER_SIMD)))
nlp_solve_fence_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, double *W, double *work, double *mult,
                       double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                       int32_t *__restrict__ status_out, int32_t *queue, d2d_wind_field wf, const double *__restrict__ t_start,
                       d2d_keep_out keep, double *kwork, d2d_fence fence, double *fwork) {
  nlp_handout_body<NLP_WIND * WIND | NLP_T_AT | NLP_KEEP | NLP_FENCE>(B, N, h, o, scen, W, work, mult, cost_out, feas_out, iters_out, status_out,
                                                                      queue, &wf, 0.0, t_start, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                      nullptr, &keep, kwork, &fence, fwork);
}

// d2d_nlp_solve_keepout_moving: outside every problem's hard discs that move -- the centre planes ctr [B][n_mov][2][N] sampled ahead
template <bool WIND>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WIND_WAVES_PER_SIMD, NLP_WIND_WAVES_PER_SIMD)))
nlp_solve_keepout_moving_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, double *W, double *work, double *mult,
                                double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                                int32_t *__restrict__ status_out, int32_t *queue, d2d_wind_field wf, const double *__restrict__ t_start,
                                d2d_moving_obstacles mv, const double *ctr, double *kwork) {
  nlp_handout_body<NLP_WIND * WIND | NLP_T_AT | NLP_KMOV>(B, N, h, o, scen, W, work, mult, cost_out, feas_out, iters_out, status_out, queue, &wf, 0.0,
                                                          t_start, &mv, ctr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kwork);
}

// d2d_nlp_solve_moving: around the problems' moving discs -- the rows' constant wind or the field (WIND), the start time per problem.
// nlp_handout_body<NLP_WIND * WIND | NLP_T_AT | NLP_MOV> written out: through the body the constant-wind instantiation took 256 VGPRs for its 255
// (DESIGN 5.16), so this kernel keeps its loop and shares the ticket, the track check and the report.
template <bool WIND>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WIND_WAVES_PER_SIMD, NLP_WIND_WAVES_PER_SIMD)))
nlp_solve_moving_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, double *W, double *work, double *mult,
                        double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                        int32_t *__restrict__ status_out, int32_t *queue, d2d_wind_field wf, const double *__restrict__ t_start,
                        d2d_moving_obstacles mv, const double *ctr) {
  const int lane = threadIdx.x;
  extern __shared__ __attribute__((aligned(16))) double nlp_lds[];
  double *wsb = work + (size_t)blockIdx.x * WS_TOTAL * N;
  const int32_t *__restrict__ order = o.order;
  for (int t = blockIdx.x; t < B;) {
    const int b = order ? __builtin_amdgcn_readfirstlane(order[t]) : t;
    if ((unsigned)b >= (unsigned)B) {        // (an entry that is no problem index is skipped, not dereferenced)
      t = nlp_next_ticket(queue, lane);
      continue;
    }
    NlpOut out;
    double t0 = 0.0;
    bool bad = false;
    if (WIND || mv.n_mov > 0) {
      t0 = nlp_first_lane(t_start[b]);
      bad = !(fabs(t0) <= 1.79e308);
    }
    if (mv.n_mov > 0) bad = bad || nlp_mov_bad(mv, b, lane);
    if (bad) {
      out.cost = out.feas = __builtin_nan(""); out.iters = 0; out.status = D2D_ST_NONFINITE;
    } else {
      const NlpMovSet ms{ctr + (size_t)b * mv.n_mov * 2 * N, mv.disc + (size_t)b * mv.n_mov * 2, mv.n_mov};
      nlp_solve_one<NLP_WIND * WIND | NLP_MOV>(N, h, o, scen + (size_t)b * D2D_SCEN_STRIDE, nullptr, W + (size_t)b * NLP_NV * N, wsb,
                                               mult ? mult + (size_t)b * 3 * N : nullptr, lane, out, nullptr, nlp_lds,
                                               o.bounds ? o.bounds + (size_t)b * 4 : nullptr, NlpExtra{{nullptr, nullptr, nullptr}, &wf, t0, 0u, &ms, nullptr});
    }
    nlp_report(b, lane, out, cost_out, feas_out, iters_out, status_out);
    nlp_phase_sync();                        // (the next problem's first stores to the workspace follow this one's last loads)
    t = nlp_next_ticket(queue, lane);
  }
}

// d2d_nlp_solve_via: nlp_solve_moving_kernel through every problem's own pins
template <bool WIND>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_WIND_WAVES_PER_SIMD, NLP_WIND_WAVES_PER_SIMD)))
nlp_solve_via_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, double *W, double *work, double *mult,
                     double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                     int32_t *__restrict__ status_out, int32_t *queue, d2d_wind_field wf, const double *__restrict__ t_start,
                     d2d_moving_obstacles mv, const double *ctr, d2d_via_points via, int32_t *vwork) {
  nlp_handout_body<NLP_WIND * WIND | NLP_T_AT | NLP_MOV | NLP_VIA>(B, N, h, o, scen, W, work, mult, cost_out, feas_out, iters_out, status_out, queue,
                                                                   &wf, 0.0, t_start, &mv, ctr, &via, vwork);
}

// A scenario of the group loop is refused: all its aircraft at once, before the workgroup's first barrier (the caller returns).
__device__ __forceinline__ void nlp_groups_refuse(int b, int r, int wave, int lane, double *cost_out, double *feas_out,
                                                  int32_t *iters_out, int32_t *status_out, int32_t *sweeps_out, double *moved_out) {
  if (lane == 0) {
    cost_out[b] = feas_out[b] = __builtin_nan("");
    if (iters_out) iters_out[b] = 0;
    if (status_out) status_out[b] = D2D_ST_NONFINITE;
    if (wave == 0) {
      if (sweeps_out) sweeps_out[r] = 0;
      if (moved_out) moved_out[r] = 0.0;
    }
  }
}

// The group loop's report: per aircraft, and per scenario by its first wavefront.
__device__ __forceinline__ void nlp_groups_report(int b, int r, int wave, int lane, const NlpOut &out, int iters_total, int sweep, double moved,
                                                  double *cost_out, double *feas_out, int32_t *iters_out, int32_t *status_out,
                                                  int32_t *sweeps_out, double *moved_out) {
  if (lane == 0) {
    cost_out[b] = out.cost;
    feas_out[b] = out.feas;
    if (iters_out) iters_out[b] = iters_total;
    if (status_out) status_out[b] = out.status;
    if (wave == 0) {
      if (sweeps_out) sweeps_out[r] = sweep;
      if (moved_out) moved_out[r] = moved;
    }
  }
}

// does aircraft a take turns in sweeps 1..?  Fixed pair: aircraft 0 and 1; PAIRS: the aircraft with a non-empty partner set (cset)
template <unsigned F>
__device__ __forceinline__ bool nlp_takes_turns(unsigned cset, int a) {
  if constexpr (NlpFeatures<F>::PAIRS) return ((cset >> a) & 1u) != 0u;
  else return a < 2;
}

// The reference's multi-aircraft Problem (src/multi_opt_planner.py:69-78,86) in ONE launch: a workgroup takes a scenario, wavefront
// a its aircraft a.  The aircraft are coupled through the objective only -- CostCollision on the pair (0, 1), src/d2d/
// multiopty_utils.py:120-153; every constraint is per aircraft -- so a fixed point of block Gauss-Seidel over the aircraft (each
// block = the full collocation solve of one aircraft against its partners' frozen node positions) is a KKT point of the joint
// problem.  Sweep 0 solves every aircraft uncoupled, concurrently; then the coupled aircraft take turns in index order (workgroup
// barriers between the turns; a partner's positions are read from its W in global memory, L2-resident, which its wave does not touch
// meanwhile) until none moved by more than tol in a sweep, or max_sweeps.  No host round trips.  prev [R][2][N] scratch.
// One body for the group kernels below, switched at compile time by F.  What the solve does with each member stands at NlpFeatures;
// what the members mean HERE, to a scenario:
// WIND: the field is shared by the launch and travels as a kernel argument (scalar registers); the start time is the SCENARIO's
//   (t_start [R], device memory: the mission chain computes it on the device), wave-uniform.  A scenario whose start time is not
//   finite is refused before its first solve.
// PAIRS: any set of coupled pairs instead of the pair (0, 1) when the row's KCOL > 0.  D2D_SC_PMASK of aircraft a's row is its
//   partner set, bit j = aircraft j of the same scenario; each turn solves against ALL partners.  With the masks of the pair (0, 1)
//   every solve, sum and barrier is that of the fixed pair (tests/test_gpu_collision_pairs.py: equal bit for bit).  The masks are checked before the scenario's
//   first solve, by every wavefront alike (scalar loads): an entry that is no integer in [0, 2^n_ac), a self bit or a bit j whose
//   aircraft j does not name a back -- the term of a pair belongs to both objectives or to none -- refuses the whole scenario
//   (D2D_ST_NONFINITE, cost = feas = NaN, sweeps = 0, W untouched), like a non-finite start time: no mask ever indexes outside the
//   scenario's W.
// MOV (d2d_nlp_solve_groups_moving): every aircraft of scenario r solves around the scenario's moving discs, centre planes
//   ctr [R][n_mov][2][N] sampled at t_start[r] + i h ahead of this launch.  The tracks are checked before the first solve, by every
//   wavefront alike; an unusable track, or a start time that is not finite while discs move, refuses the scenario like a bad mask.
// VIA (d2d_nlp_solve_groups_via): every AIRCRAFT has its own pins, via->pts [R n_ac][n_via][5], and its own plane vwork [R n_ac][N].  The
//   pins of all aircraft are checked before the first solve, by every wavefront alike: one unusable row refuses the scenario.
// The pointer parameters of the body and of its two helpers carry no __restrict__ (the kernels' do): with it the fixed-pair kernel
// went from 256 VGPRs / 624 B of scratch to 255 / 608 and the field kernel from 752 B to 784.
// Registers: 512 threads per workgroup are 8 wavefronts on 4 SIMDs, two per SIMD, so a wavefront gets at most 256 of the SIMD's 512
// registers whatever amdgpu_waves_per_eu says -- the workgroup size binds, and (2, 2) states what the hardware does.
// KMOV (d2d_nlp_solve_groups_keepout): mv and ctr are the scenario's HARD moving discs (NlpKeepMovSet), held by every aircraft in the
//   uncoupled sweep and in every turn; kwork [R n_ac][n_mov][N] the planes of their duals, every aircraft its own.  Tracks, radii and the
//   start time are checked like MOV's; an aircraft whose end pose lies inside a disc or that the start rule cannot place outside the
//   discs refuses the SCENARIO -- every wavefront checks every aircraft of the scenario, before the first barrier, as VIA checks the pins.
// FENCE (d2d_nlp_solve_groups_fence): fence->edges [R][n_edge][4] is the SCENARIO's polygon, held by every aircraft in the uncoupled sweep
//   and in every turn; fwork [R n_ac][n_edge][N] the planes of the duals, every aircraft its own.  No hard discs.  An unusable edge, or an
//   aircraft whose end pose lies on or outside an edge or that the start rule cannot place inside, refuses the SCENARIO -- every wavefront
//   checks every aircraft, before the first barrier, as KMOV does.  A later turn that cannot start refuses that aircraft alone.
template <unsigned F>
__device__ __forceinline__ void nlp_groups_body(int R, int n_ac, int N, double h, const d2d_nlp_opts &o, int max_sweeps, double tol,
                                                const double *scen, double *W, double *work, double *mult, double *prev,
                                                double *cost_out, double *feas_out, int32_t *iters_out, int32_t *status_out, int32_t *sweeps_out,
                                                double *moved_out, const d2d_wind_field *wf, const double *t_start,
                                                const d2d_moving_obstacles *mv = nullptr, const double *ctr = nullptr, const d2d_via_points *via = nullptr,
                                                int32_t *vwork = nullptr, [[maybe_unused]] double *kwork = nullptr,
                                                [[maybe_unused]] const d2d_fence *fence = nullptr, [[maybe_unused]] double *fwork = nullptr) {
  NLP_FEATURES(F);
  static_assert(!(MODEL || FREE || T_AT) && (!KEEP || KMOV), "the group loop holds moving hard discs or a polygon, under the structured objective");
  __shared__ double moved_s[PAIRS ? 8 : 2];
  extern __shared__ __attribute__((aligned(16))) double nlp_lds[];
  const int r = blockIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int b = r * n_ac + wave;
  double t0 = 0.0;
  bool bad = false;
  if constexpr (WIND) {
    t0 = nlp_first_lane(t_start[r]);
    bad = !(fabs(t0) <= 1.79e308);
  }
  unsigned cset = 0u, pmask = 0u;            // PAIRS: the aircraft that take turns; this aircraft's partner set
  if constexpr (PAIRS) {
    unsigned long long masks = 0ull;         // the scenario's masks, 8 bits per aircraft
    for (int a = 0; a < n_ac; ++a) {
      const double pm = scen[(size_t)(r * n_ac + a) * D2D_SCEN_STRIDE + D2D_SC_PMASK];
      if (!(pm >= 0.0 && pm < (double)(1u << n_ac)) || pm != floor(pm)) { bad = true; continue; }
      const unsigned m = (unsigned)pm;
      if ((m >> a) & 1u) bad = true;
      masks |= (unsigned long long)m << (8 * a);
      if (m != 0u) cset |= 1u << a;
    }
    for (int a = 0; a < n_ac; ++a)
      for (int j = 0; j < n_ac; ++j)
        if (((masks >> (8 * a + j)) & 1ull) != ((masks >> (8 * j + a)) & 1ull)) bad = true;
    bad = __builtin_amdgcn_readfirstlane((int)bad) != 0;
    cset = (unsigned)__builtin_amdgcn_readfirstlane((int)cset);
    pmask = (unsigned)__builtin_amdgcn_readfirstlane((int)((masks >> (8 * wave)) & 0xffull));
  }
  [[maybe_unused]] NlpMovSet ms{nullptr, nullptr, 0};
  const NlpMovSet *msp = nullptr;
  if constexpr (MOV) {
    if (mv->n_mov > 0) {
      if constexpr (!WIND) bad = bad || !(fabs(nlp_first_lane(t_start[r])) <= 1.79e308);
      bad = bad || nlp_mov_bad(*mv, r, lane);
    }
    ms = NlpMovSet{ctr + (size_t)r * mv->n_mov * 2 * N, mv->disc + (size_t)r * mv->n_mov * 2, mv->n_mov};
    msp = &ms;
  }
  [[maybe_unused]] NlpViaSet vs{nullptr, nullptr, 0};
  const NlpViaSet *vsp = nullptr;
  if constexpr (VIA) {
    for (int a = 0; a < n_ac; ++a) {
      const size_t ba = (size_t)r * n_ac + a;
      bad = bad || nlp_via_bad(via->pts + ba * via->n_via * 5, via->n_via, N, scen + ba * D2D_SCEN_STRIDE, o, o.bounds ? o.bounds + ba * 4 : nullptr, lane);
    }
    vs = NlpViaSet{via->pts + (size_t)b * via->n_via * 5, vwork + (size_t)b * N, via->n_via};
    vsp = &vs;
  }
  [[maybe_unused]] NlpKeepMovSet kms{{nullptr, nullptr, 0}, nullptr};
  if constexpr (KMOV) {
    if (mv->n_mov > 0) {
      if constexpr (!WIND) bad = bad || !(fabs(nlp_first_lane(t_start[r])) <= 1.79e308);
      bad = bad || nlp_mov_bad(*mv, r, lane);
    }
    kms = NlpKeepMovSet{{mv->disc + (size_t)r * mv->n_mov * 2, kwork + (size_t)b * mv->n_mov * N, mv->n_mov}, ctr + (size_t)r * mv->n_mov * 2 * N};
    if (!bad && mv->n_mov > 0) {             // (the centre planes are read only behind a good track)
      for (int a = 0; a < n_ac; ++a) {
        const size_t ba = (size_t)r * n_ac + a;
        const double *sca = scen + ba * D2D_SCEN_STRIDE;
        const NlpScen sa = nlp_load_scen(sca, o, o.bounds ? o.bounds + ba * 4 : nullptr);
        bad = bad || nlp_keep_bad(sa, kms, W + ba * NLP_NV * N, N, lane);
      }
    }
    __syncthreads();                         // (every wavefront has read every aircraft's start before the first solve writes one)
  }
  [[maybe_unused]] NlpKeepFenceSet kfs{{nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
  if constexpr (FENCE) {
    kfs.fence = NlpFenceSet{fence->edges + (size_t)r * fence->n_edge * 4, fwork + (size_t)b * fence->n_edge * N, fence->n_edge};
    if (!bad) {
      NlpFenceProb fp;                       // (nlp_fence_bad<NLP_FENCE> reads its fence alone)
      fp.fence = kfs.fence;
      for (int a = 0; a < n_ac; ++a) {
        const size_t ba = (size_t)r * n_ac + a;
        const NlpScen sa = nlp_load_scen(scen + ba * D2D_SCEN_STRIDE, o, o.bounds ? o.bounds + ba * 4 : nullptr);
        bad = bad || nlp_fence_bad<NLP_FENCE>(sa, fp, W + ba * NLP_NV * N, N, lane);
      }
    }
    __syncthreads();                         // (every wavefront has read every aircraft's start before the first solve writes one)
  }
  if (bad) {                                 // (uniform over the workgroup: before the first barrier)
    nlp_groups_refuse(b, r, wave, lane, cost_out, feas_out, iters_out, status_out, sweeps_out, moved_out);
    return;
  }
  const double *sc = scen + (size_t)b * D2D_SCEN_STRIDE;
  double *Wb = W + (size_t)b * NLP_NV * N;
  double *wsb = work + (size_t)b * WS_TOTAL * N;
  double *mb = mult ? mult + (size_t)b * 3 * N : nullptr;
  const double *Wr = W + (size_t)r * n_ac * NLP_NV * N;        // the scenario's W: aircraft j's planes at j * 5 * N
  bool coupled;                              // wave-uniform for the whole group
  if constexpr (PAIRS) coupled = cset != 0u;
  else coupled = n_ac >= 2 && scen[(size_t)(r * n_ac) * D2D_SCEN_STRIDE + D2D_SC_KCOL] > 0.0;
  NlpOut out;
  int iters_total = 0;
  double *ldsw = nlp_lds + (size_t)wave * NLP_LDS_DOUBLES;
  const double *bnd = o.bounds ? o.bounds + (size_t)b * 4 : nullptr;
  NlpExtra ex{{nullptr, nullptr, nullptr}, wf, t0, 0u, msp, vsp};      // sweep 0: no partner
  if constexpr (KMOV) ex.keep = &kms;
  if constexpr (FENCE) ex.keep = &kfs;
  nlp_solve_one<F>(N, h, o, sc, PAIRS ? Wr : nullptr, Wb, wsb, mb, lane, out, nullptr, ldsw, bnd, ex);
  ex.pmask = pmask;
  iters_total += out.iters;
  if (threadIdx.x < (PAIRS ? 8 : 2)) moved_s[threadIdx.x] = 0.0;
  __threadfence_block();
  __syncthreads();
  int sweep = 0;
  double moved = 0.0;
  if (coupled) {
    double *pv = prev + (size_t)r * 2 * N;
    const int n_turns = PAIRS ? n_ac : 2;
    for (sweep = 1; sweep <= max_sweeps; ++sweep) {
      for (int turn = 0; turn < n_turns; ++turn) {
        if (!nlp_takes_turns<F>(cset, turn)) continue;
        if (wave == turn) {
          // fixed pair: the partner's x and y planes; PAIRS: the scenario's W and the set
          const double *pw = PAIRS ? Wr : W + (size_t)(r * n_ac + (1 - turn)) * NLP_NV * N;
          for (int i = lane; i < 2 * N; i += 64) pv[i] = Wb[i];
          nlp_solve_one<F>(N, h, o, sc, pw, Wb, wsb, mb, lane, out, nullptr, ldsw, bnd, ex);
          iters_total += out.iters;
          double m = 0.0;
          for (int i = lane; i < 2 * N; i += 64) m = fmax(m, fabs(Wb[i] - pv[i]));
          m = wave_max(m);
          if (lane == 0) moved_s[turn] = m;
        }
        __threadfence_block();
        __syncthreads();
      }
      if constexpr (PAIRS) {
        moved = 0.0;
        for (int a = 0; a < n_ac; ++a) moved = fmax(moved, moved_s[a]);     // (the entries of aircraft outside cset stay 0)
      } else {
        moved = fmax(moved_s[0], moved_s[1]);
      }
      __syncthreads();
      if (moved <= tol) break;
    }
    if (sweep > max_sweeps) sweep = max_sweeps;
    // not settled after the last sweep: the coupled aircraft are reported as such (the inner solves each converged, the alternation did not)
    if (moved > tol && nlp_takes_turns<F>(cset, wave) && out.status == D2D_ST_CONVERGED) out.status = D2D_ST_MAXITER;
  }
  nlp_groups_report(b, r, wave, lane, out, iters_total, sweep, moved, cost_out, feas_out, iters_out, status_out, sweeps_out, moved_out);
}

#ifndef NLP_GROUPS_WIND_WAVES_PER_SIMD
#define NLP_GROUPS_WIND_WAVES_PER_SIMD 2
#endif
// d2d_nlp_solve_groups: the pair (0, 1), the rows' constant wind
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NLP_WAVES_PER_SIMD, NLP_WAVES_PER_SIMD)))
nlp_groups_kernel(int R, int n_ac, int N, double h, d2d_nlp_opts o, int max_sweeps, double tol, const double *__restrict__ scen, double *W,
                  double *work, double *mult, double *prev, double *__restrict__ cost_out, double *__restrict__ feas_out,
                  int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out, int32_t *__restrict__ sweeps_out,
                  double *__restrict__ moved_out) {
  nlp_groups_body<0u>(R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, prev, cost_out, feas_out, iters_out, status_out, sweeps_out, moved_out,
                      nullptr, nullptr);
}

// d2d_nlp_solve_groups_wind: the pair (0, 1) in a field
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NLP_GROUPS_WIND_WAVES_PER_SIMD, NLP_GROUPS_WIND_WAVES_PER_SIMD)))
nlp_groups_wind_kernel(int R, int n_ac, int N, double h, d2d_nlp_opts o, int max_sweeps, double tol, const double *__restrict__ scen, double *W,
                       double *work, double *mult, double *prev, double *__restrict__ cost_out, double *__restrict__ feas_out,
                       int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out, int32_t *__restrict__ sweeps_out,
                       double *__restrict__ moved_out, d2d_wind_field wf, const double *__restrict__ t_start) {
  nlp_groups_body<NLP_WIND>(R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, prev, cost_out, feas_out, iters_out, status_out, sweeps_out,
                            moved_out, &wf, t_start);
}

// d2d_nlp_solve_groups_pairs: the pairs of the masks; WIND selects the rows' constant wind or the field
template <bool WIND>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NLP_GROUPS_WIND_WAVES_PER_SIMD, NLP_GROUPS_WIND_WAVES_PER_SIMD)))
nlp_groups_pairs_kernel(int R, int n_ac, int N, double h, d2d_nlp_opts o, int max_sweeps, double tol, const double *__restrict__ scen, double *W,
                        double *work, double *mult, double *prev, double *__restrict__ cost_out, double *__restrict__ feas_out,
                        int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out, int32_t *__restrict__ sweeps_out,
                        double *__restrict__ moved_out, d2d_wind_field wf, const double *__restrict__ t_start) {
  nlp_groups_body<NLP_WIND * WIND | NLP_PAIRS>(R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, prev, cost_out, feas_out, iters_out, status_out,
                                               sweeps_out, moved_out, &wf, t_start);
}

// d2d_nlp_solve_groups_moving: the pairs of the masks around the scenarios' moving discs; WIND as above
template <bool WIND>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NLP_GROUPS_WIND_WAVES_PER_SIMD, NLP_GROUPS_WIND_WAVES_PER_SIMD)))
nlp_groups_moving_kernel(int R, int n_ac, int N, double h, d2d_nlp_opts o, int max_sweeps, double tol, const double *__restrict__ scen, double *W,
                         double *work, double *mult, double *prev, double *__restrict__ cost_out, double *__restrict__ feas_out,
                         int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out, int32_t *__restrict__ sweeps_out,
                         double *__restrict__ moved_out, d2d_wind_field wf, const double *__restrict__ t_start, d2d_moving_obstacles mv,
                         const double *__restrict__ ctr) {
  nlp_groups_body<NLP_WIND * WIND | NLP_PAIRS | NLP_MOV>(R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, prev, cost_out, feas_out, iters_out,
                                                         status_out, sweeps_out, moved_out, &wf, t_start, &mv, ctr);
}

// d2d_nlp_solve_groups_keepout: the pairs of the masks, every aircraft outside the scenario's hard moving discs; WIND as above
template <bool WIND>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NLP_GROUPS_WIND_WAVES_PER_SIMD, NLP_GROUPS_WIND_WAVES_PER_SIMD)))
nlp_groups_keepout_kernel(int R, int n_ac, int N, double h, d2d_nlp_opts o, int max_sweeps, double tol, const double *__restrict__ scen, double *W,
                          double *work, double *mult, double *prev, double *__restrict__ cost_out, double *__restrict__ feas_out,
                          int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out, int32_t *__restrict__ sweeps_out,
                          double *__restrict__ moved_out, d2d_wind_field wf, const double *__restrict__ t_start, d2d_moving_obstacles mv,
                          const double *__restrict__ ctr, double *kwork) {
  nlp_groups_body<NLP_WIND * WIND | NLP_PAIRS | NLP_KMOV>(R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, prev, cost_out, feas_out, iters_out,
                                                          status_out, sweeps_out, moved_out, &wf, t_start, &mv, ctr, nullptr, nullptr, kwork);
}

// d2d_nlp_solve_groups_fence: the pairs of the masks, every aircraft inside the scenario's convex polygon; WIND as above
template <bool WIND>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NLP_GROUPS_WIND_WAVES_PER_SIMD, NLP_GROUPS_WIND_WAVES_PER_SIMD)))
nlp_groups_fence_kernel(int R, int n_ac, int N, double h, d2d_nlp_opts o, int max_sweeps, double tol, const double *__restrict__ scen, double *W,
                        double *work, double *mult, double *prev, double *__restrict__ cost_out, double *__restrict__ feas_out,
                        int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out, int32_t *__restrict__ sweeps_out,
                        double *__restrict__ moved_out, d2d_wind_field wf, const double *__restrict__ t_start, d2d_fence fence, double *fwork) {
  nlp_groups_body<NLP_WIND * WIND | NLP_PAIRS | NLP_FENCE>(R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, prev, cost_out, feas_out, iters_out,
                                                           status_out, sweeps_out, moved_out, &wf, t_start, nullptr, nullptr, nullptr, nullptr,
                                                           nullptr, &fence, fwork);
}

// d2d_nlp_solve_groups_via: the pairs of the masks around the scenarios' moving discs, through every aircraft's own pins; WIND as above
template <bool WIND>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NLP_GROUPS_WIND_WAVES_PER_SIMD, NLP_GROUPS_WIND_WAVES_PER_SIMD)))
nlp_groups_via_kernel(int R, int n_ac, int N, double h, d2d_nlp_opts o, int max_sweeps, double tol, const double *__restrict__ scen, double *W,
                      double *work, double *mult, double *prev, double *__restrict__ cost_out, double *__restrict__ feas_out,
                      int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out, int32_t *__restrict__ sweeps_out,
                      double *__restrict__ moved_out, d2d_wind_field wf, const double *__restrict__ t_start, d2d_moving_obstacles mv,
                      const double *__restrict__ ctr, d2d_via_points via, int32_t *vwork) {
  nlp_groups_body<NLP_WIND * WIND | NLP_PAIRS | NLP_MOV | NLP_VIA>(R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, prev, cost_out, feas_out,
                                                                   iters_out, status_out, sweeps_out, moved_out, &wf, t_start, &mv, ctr, &via, vwork);
}

// d2d_nlp_solve_model: the collocation NLP under the quadratic objective model of a cost that only the host can evaluate (a user's
// cost plug-in, opty/direct_collocation.py).  One wavefront and one workspace per problem: the launch holds the few aircraft of one
// Problem, so there is nothing to hand out and no second wave per SIMD to fill: it runs at one wave per SIMD (256 VGPRs + 74 AGPRs,
// 240 B / lane of scratch -- what nlp_solve_kernel built for one wave has too -- against 528 B / lane at two; DESIGN measured one
// wave per SIMD at the same speed for this solver).
#ifndef NLP_MODEL_WAVES_PER_SIMD
#define NLP_MODEL_WAVES_PER_SIMD 1
#endif
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NLP_MODEL_WAVES_PER_SIMD, NLP_MODEL_WAVES_PER_SIMD)))
nlp_model_kernel(int B, int N, double h, d2d_nlp_opts o, const double *__restrict__ scen, d2d_nlp_model m, double *W, double *work,
                 double *mult, double *__restrict__ cost_out, double *__restrict__ feas_out, int32_t *__restrict__ iters_out,
                 int32_t *__restrict__ status_out) {
  const int lane = threadIdx.x, b = blockIdx.x;
  extern __shared__ __attribute__((aligned(16))) double nlp_lds[];
  const size_t pl = (size_t)b * N;
  const NlpModel md{m.g + pl * NLP_NV, m.H + pl * 15, m.Wc + pl * NLP_NV};
  NlpOut out;
  nlp_solve_one<NLP_MODEL>(N, h, o, scen + (size_t)b * D2D_SCEN_STRIDE, nullptr, W + pl * NLP_NV, work + pl * WS_TOTAL, mult ? mult + pl * 3 : nullptr,
                      lane, out, nullptr, nlp_lds, o.bounds ? o.bounds + (size_t)b * 4 : nullptr, NlpExtra{md});
  if (lane == 0) {
    cost_out[b] = out.cost;
    feas_out[b] = out.feas;
    if (iters_out) iters_out[b] = out.iters;
    if (status_out) status_out[b] = out.status;
  }
}

// D2D_NLP_STAMPS (diagnostics): the buffer of problem 0's cycle stamps, or null; nlp_stamps_report prints and frees it (synchronous)
static int nlp_stamps_alloc(unsigned long long **stamps) {
  *stamps = nullptr;
  if (getenv("D2D_NLP_STAMPS")) D2D_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(stamps), 16 * sizeof(unsigned long long)));
  return D2D_OK;
}
static int nlp_stamps_report(d2d_ctx *ctx, unsigned long long *stamps) {
  if (!stamps) return D2D_OK;
  unsigned long long hs[9];
  D2D_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  D2D_CHECK_HIP(hipMemcpy(hs, stamps, sizeof(hs), hipMemcpyDeviceToHost));
  D2D_CHECK_HIP(hipFree(stamps));
  static const char *nm[8] = {"merit", "assemble", "factor", "backsolve", "recover+ratio tests", "update", "eliminate", "other"};
  fprintf(stderr, "[nlp] problem 0: %llu Newton steps; shader clocks per phase:", hs[8]);
  for (int k = 0; k < 8; ++k) fprintf(stderr, " %s %llu", nm[k], hs[k]);
  fprintf(stderr, "\n");
  return D2D_OK;
}

// opts or the defaults, validated; who: the entry's name for the message
static int nlp_options(const d2d_nlp_opts *opts, const char *who, d2d_nlp_opts *o) {
  *o = {D2D_NLP_RHO0, D2D_NLP_MUB0, D2D_NLP_MUB_MIN, 1e-9, 1e-7, 60, 40, 0, 0, nullptr, nullptr};
  if (opts) *o = *opts;
  D2D_REQUIRE(o->inner_max >= 1 && o->outer_max >= 1 && o->rho0 > 0 && o->mub0 > 0 && o->mub_min > 0, "%s: bad options", who);
  return D2D_OK;
}

// the persistent launches' grid: one wavefront per wave slot of the chip (d2d_nlp_opts.slots > 0: the caller's count), or per problem
static int nlp_handout_grid(int B, const d2d_nlp_opts &o, int waves_per_simd) {
  static int n_cu = 0;
  if (n_cu == 0) { int dev = 0; (void)hipGetDevice(&dev); if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) n_cu = 256; }
  int slots = n_cu * 4 * waves_per_simd;
  if (o.slots > 0) slots = o.slots;
  return B < slots ? B : (slots < 1 ? 1 : slots);
}

// what the single-problem entries require alike
static int nlp_single_check(const d2d_ctx *ctx, int B, int N, double h, const double *scen, const double *W, const double *work,
                            const double *cost, const double *feas, const char *who) {
  D2D_REQUIRE(ctx && scen && W && work && cost && feas, "%s: null argument", who);
  D2D_REQUIRE(B >= 1 && N >= 3 && h > 0, "%s: B >= 1, N >= 3, h > 0 required (B=%d N=%d h=%g)", who, B, N, h);
  return D2D_OK;
}

// the optional field of an entry: f and t_start go together -- when discs move (mov: the entry's table, null if it takes none) the
// start times are there already (check_moving) and the field alone is optional
static int nlp_field_check(const d2d_wind_field *f, const double *t_start, const d2d_moving_obstacles *mov, const char *who) {
  if (!mov)
    D2D_REQUIRE((f == nullptr) == (t_start == nullptr), "%s: f and t_start go together (both NULL: the rows' constant wind)", who);
  else if (mov->n_mov == 0)
    D2D_REQUIRE((f == nullptr) == (t_start == nullptr), "%s: without moving discs f and t_start go together (both NULL: the rows' constant wind)", who);
  return f ? check_wind(f, who) : D2D_OK;
}

// f or no f: launch(WIND as a std::bool_constant, the field's kernel argument), so that an entry names its kernel template once
template <typename Launch>
static int nlp_with_field(const d2d_wind_field *f, Launch launch) {
  return f ? launch(std::true_type{}, *f) : launch(std::false_type{}, d2d_wind_field{});
}

// a hand-out kernel's launch: the grid, the queue's reset, a wavefront and an LDS block per slot; tail: what follows the queue
template <typename Kernel, typename... Tail>
static int nlp_handout_launch(Kernel kernel, d2d_ctx *ctx, int B, int N, double h, const d2d_nlp_opts &o, const double *scen, double *W,
                              double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, Tail... tail) {
  const int grid = nlp_handout_grid(B, o, NLP_WIND_WAVES_PER_SIMD);
  int32_t *queue = ctx->counter_dev + 2;
  D2D_CHECK_HIP(hipMemsetAsync(queue, 0, sizeof(int32_t), ctx->stream));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), NLP_LDS_DOUBLES * sizeof(double), ctx->stream, B, N, h, o, scen, W, work, mult, cost, feas, iters,
                     status, queue, tail...);
  D2D_LAUNCH_CHECK();
  return D2D_OK;
}

// the group loops' scratch for the positions before a turn: the tail of aircraft 0's workspace is not free, so it lives behind the workspaces
static double *nlp_groups_prev(double *work, int R, int n_ac, int N) { return work + (size_t)R * n_ac * WS_TOTAL * N; }

// what the group entries require alike
static int nlp_groups_check(const d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, int max_sweeps, double tol,
                            const double *W, const double *work, const double *cost, const double *feas, const char *who) {
  D2D_REQUIRE(ctx && scen && W && work && cost && feas, "%s: null argument", who);
  D2D_REQUIRE(R >= 1 && n_ac >= 1 && n_ac <= 8 && N >= 3 && h > 0, "%s: R >= 1, 1 <= n_ac <= 8, N >= 3, h > 0 required (R=%d n_ac=%d N=%d h=%g)", who, R, n_ac, N, h);
  D2D_REQUIRE(max_sweeps >= 1 && tol >= 0, "%s: max_sweeps >= 1 and tol >= 0 required", who);
  return D2D_OK;
}

// a group kernel's launch: a workgroup per scenario, a wavefront and an LDS block per aircraft
template <typename Kernel, typename... Args>
static int nlp_groups_launch(Kernel kernel, d2d_ctx *ctx, int R, int n_ac, Args... args) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * NLP_LDS_DOUBLES * (int)sizeof(double));
  hipLaunchKernelGGL(kernel, dim3(R), dim3(64 * n_ac), (size_t)n_ac * NLP_LDS_DOUBLES * sizeof(double), ctx->stream, R, n_ac, args...);
  D2D_LAUNCH_CHECK();
  return D2D_OK;
}

// a d2d_moving_obstacles argument of an entry point (include/d2d.h: what makes one D2D_EINVAL); work: the centre planes
static int check_moving(const d2d_moving_obstacles *mov, const double *work, const double *t_start, const char *who) {
  D2D_REQUIRE(mov, "%s: null moving-obstacle table (n_mov = 0: nothing moves)", who);
  D2D_REQUIRE(mov->n_mov >= 0 && mov->n_mov <= D2D_MAX_MOV, "%s: n_mov = %d outside 0 .. %d", who, mov->n_mov, D2D_MAX_MOV);
  if (mov->n_mov == 0) return D2D_OK;
  D2D_REQUIRE(mov->n_knot >= 2 && mov->n_knot <= D2D_MOV_MAX_KNOT, "%s: n_knot = %d outside 2 .. %d", who, mov->n_knot, D2D_MOV_MAX_KNOT);
  D2D_REQUIRE(mov->knots && mov->disc, "%s: null knots or disc table with n_mov = %d", who, mov->n_mov);
  D2D_REQUIRE(work, "%s: null array of centre planes with n_mov = %d", who, mov->n_mov);
  D2D_REQUIRE(t_start, "%s: null t_start with n_mov = %d (a device array: the tracks' times are absolute)", who, mov->n_mov);
  return D2D_OK;
}

// a d2d_via_points argument of an entry point (include/d2d.h: what makes one D2D_EINVAL); work: the planes of the fixed sets
static int check_via(const d2d_via_points *via, const int32_t *work, const char *who) {
  D2D_REQUIRE(via, "%s: null via-point table (n_via = 0: no pins)", who);
  D2D_REQUIRE(via->n_via >= 0 && via->n_via <= D2D_MAX_VIA, "%s: n_via = %d outside 0 .. %d", who, via->n_via, D2D_MAX_VIA);
  if (via->n_via == 0) return D2D_OK;
  D2D_REQUIRE(via->pts, "%s: null table with n_via = %d", who, via->n_via);
  D2D_REQUIRE(work, "%s: null via_work with n_via = %d", who, via->n_via);
  return D2D_OK;
}

// the sampler's launch on the context's stream, if anything moves: a workgroup per (problem or scenario, disc)
static int nlp_mov_sample_launch(d2d_ctx *ctx, int G, int N, double h, const double *t_start, const d2d_moving_obstacles &mov, double *ctr) {
  if (mov.n_mov == 0) return D2D_OK;
  hipLaunchKernelGGL(nlp_mov_sample_kernel, dim3((unsigned)G * (unsigned)mov.n_mov), dim3(64), 0, ctx->stream, N, h, t_start, mov, ctr);
  D2D_LAUNCH_CHECK();
  return D2D_OK;
}

// what the moving and via entries of either launch shape do between their argument check and their launch: the tracks, the optional
// field, the options, the sampler
static int nlp_moving_prologue(d2d_ctx *ctx, int G, int N, double h, const d2d_nlp_opts *opts, const d2d_wind_field *f, const double *t_start,
                               const d2d_moving_obstacles *mov, double *mov_work, const char *who, d2d_nlp_opts *o) {
  if (int rc = check_moving(mov, mov_work, t_start, who)) return rc;
  if (int rc = nlp_field_check(f, t_start, mov, who)) return rc;
  if (int rc = nlp_options(opts, who, o)) return rc;
  return nlp_mov_sample_launch(ctx, G, N, h, t_start, *mov, mov_work);
}

extern "C" {

int d2d_nlp_workspace_doubles(int N) { return N * WS_TOTAL; }

int d2d_nlp_solve_model(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, const d2d_nlp_model *model,
                        double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status) {
  D2D_REQUIRE(ctx && scen && model && model->g && model->H && model->Wc && W && work && cost && feas, "d2d_nlp_solve_model: null argument");
  D2D_REQUIRE(B >= 1 && N >= 3 && h > 0, "d2d_nlp_solve_model: B >= 1, N >= 3, h > 0 required (B=%d N=%d h=%g)", B, N, h);
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_model", &o)) return rc;
  o.order = nullptr;                                       // (one wavefront per problem: no hand-out)
  hipLaunchKernelGGL(nlp_model_kernel, dim3(B), dim3(64), NLP_LDS_DOUBLES * sizeof(double), ctx->stream, B, N, h, o, scen, *model, W, work,
                     mult, cost, feas, iters, status);
  D2D_LAUNCH_CHECK();
  return D2D_OK;
}

int d2d_nlp_solve(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W,
                  const double *partner, double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status) {
  D2D_REQUIRE(ctx && scen && W && work && cost && feas, "d2d_nlp_solve: null argument");
  D2D_REQUIRE(B >= 1 && N >= 3 && h > 0, "d2d_nlp_solve: B >= 1, N >= 3, h > 0 required (B=%d N=%d h=%g)", B, N, h);
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve", &o)) return rc;
  unsigned long long *stamps;
  if (int rc = nlp_stamps_alloc(&stamps)) return rc;
  const int grid = nlp_handout_grid(B, o, NLP_WAVES_PER_SIMD);
  int32_t *queue = ctx->counter_dev + 2;
  D2D_CHECK_HIP(hipMemsetAsync(queue, 0, sizeof(int32_t), ctx->stream));
  hipLaunchKernelGGL(nlp_solve_kernel, dim3(grid), dim3(64), NLP_LDS_DOUBLES * sizeof(double), ctx->stream, B, N, h, o, scen, partner, W, work, mult, cost, feas, iters,
                     status, stamps, queue);
  D2D_LAUNCH_CHECK();
  return nlp_stamps_report(ctx, stamps);                   // diagnostics: synchronous
}

int d2d_nlp_solve_wind(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W, double *work,
                       double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, const d2d_wind_field *f, double t_start) {
  if (int rc = nlp_single_check(ctx, B, N, h, scen, W, work, cost, feas, "d2d_nlp_solve_wind")) return rc;
  D2D_REQUIRE(fabs(t_start) <= 1.79e308, "d2d_nlp_solve_wind: t_start must be finite");
  if (int rc = check_wind(f, "d2d_nlp_solve_wind")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_wind", &o)) return rc;
  return nlp_handout_launch(nlp_solve_wind_kernel, ctx, B, N, h, o, scen, W, work, mult, cost, feas, iters, status, *f, t_start);
}

int d2d_nlp_free_workspace_doubles(int N) { return N * WSF_TOTAL; }

int d2d_nlp_solve_free(d2d_ctx *ctx, int B, int N, double h0, const double *scen, const d2d_nlp_opts *opts, const double *free_rows,
                       double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, double *h_out) {
  if (int rc = nlp_single_check(ctx, B, N, h0, scen, W, work, cost, feas, "d2d_nlp_solve_free")) return rc;
  D2D_REQUIRE(free_rows && h_out, "d2d_nlp_solve_free: null free_rows or h_out");
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_free", &o)) return rc;
  D2D_REQUIRE(o.serial == 0, "d2d_nlp_solve_free: opts->serial = 1 (the twisted recursion) is not available with a free time step");
  unsigned long long *stamps;
  if (int rc = nlp_stamps_alloc(&stamps)) return rc;
  if (int rc = nlp_handout_launch(nlp_solve_free_kernel, ctx, B, N, h0, o, scen, W, work, mult, cost, feas, iters, status, free_rows, h_out, stamps))
    return rc;
  return nlp_stamps_report(ctx, stamps);                   // (factor: both passes of the cyclic reduction)
}

int d2d_nlp_solve_free_fence(d2d_ctx *ctx, int B, int N, double h0, const double *scen, const d2d_nlp_opts *opts, const double *free_rows,
                             double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, double *h_out,
                             const d2d_keep_out *keep, double *kwork, const d2d_fence *fence, double *fwork) {
  const char *who = "d2d_nlp_solve_free_fence";
  D2D_REQUIRE(fence, "%s: null fence (n_edge = 0: no edges)", who);
  D2D_REQUIRE(fence->n_edge >= 0 && fence->n_edge <= D2D_MAX_FENCE, "%s: n_edge = %d outside 0 .. %d", who, fence->n_edge, D2D_MAX_FENCE);
  D2D_REQUIRE(fence->n_edge == 0 || (fence->edges && fwork), "%s: null edges or fwork with n_edge = %d", who, fence->n_edge);
  D2D_REQUIRE(keep, "%s: null keep-out table (n_keep = 0: no discs)", who);
  D2D_REQUIRE(keep->n_keep >= 0 && keep->n_keep <= D2D_MAX_KEEP, "%s: n_keep = %d outside 0 .. %d", who, keep->n_keep, D2D_MAX_KEEP);
  D2D_REQUIRE(keep->n_keep == 0 || (keep->discs && kwork), "%s: null discs or kwork with n_keep = %d", who, keep->n_keep);
  if (keep->n_keep == 0 && fence->n_edge == 0)             // neither family: the solve of d2d_nlp_solve_free, its kernel and its checks
    return d2d_nlp_solve_free(ctx, B, N, h0, scen, opts, free_rows, W, work, mult, cost, feas, iters, status, h_out);
  if (int rc = nlp_single_check(ctx, B, N, h0, scen, W, work, cost, feas, who)) return rc;
  D2D_REQUIRE(free_rows && h_out, "%s: null free_rows or h_out", who);
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, who, &o)) return rc;
  D2D_REQUIRE(o.serial == 0, "%s: opts->serial = 1 (the twisted recursion) is not available with a free time step", who);
  return nlp_handout_launch(nlp_solve_free_fence_kernel, ctx, B, N, h0, o, scen, W, work, mult, cost, feas, iters, status, free_rows, h_out, *keep,
                            kwork, *fence, fwork);
}

int d2d_nlp_solve_groups(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                         double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters, int32_t *status,
                         int32_t *sweeps, double *moved) {
  if (int rc = nlp_groups_check(ctx, R, n_ac, N, h, scen, max_sweeps, tol, W, work, cost, feas, "d2d_nlp_solve_groups")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_groups", &o)) return rc;
  return nlp_groups_launch(nlp_groups_kernel, ctx, R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, nlp_groups_prev(work, R, n_ac, N), cost,
                           feas, iters, status, sweeps, moved);
}

int d2d_nlp_solve_groups_wind(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                              double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                              int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start) {
  if (int rc = nlp_groups_check(ctx, R, n_ac, N, h, scen, max_sweeps, tol, W, work, cost, feas, "d2d_nlp_solve_groups_wind")) return rc;
  if (int rc = check_wind(f, "d2d_nlp_solve_groups_wind")) return rc;
  D2D_REQUIRE(t_start, "d2d_nlp_solve_groups_wind: null t_start (a device array [R]: one start time per scenario)");
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_groups_wind", &o)) return rc;
  return nlp_groups_launch(nlp_groups_wind_kernel, ctx, R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult, nlp_groups_prev(work, R, n_ac, N),
                           cost, feas, iters, status, sweeps, moved, *f, t_start);
}

int d2d_nlp_solve_groups_pairs(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                               double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                               int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start) {
  if (int rc = nlp_groups_check(ctx, R, n_ac, N, h, scen, max_sweeps, tol, W, work, cost, feas, "d2d_nlp_solve_groups_pairs")) return rc;
  if (int rc = nlp_field_check(f, t_start, nullptr, "d2d_nlp_solve_groups_pairs")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_groups_pairs", &o)) return rc;
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_groups_launch(nlp_groups_pairs_kernel<decltype(wind)::value>, ctx, R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult,
                             nlp_groups_prev(work, R, n_ac, N), cost, feas, iters, status, sweeps, moved, wf, t_start);
  });
}

int d2d_mov_sample(d2d_ctx *ctx, int G, int N, double h, const double *t_start, const d2d_moving_obstacles *mov, double *ctr) {
  D2D_REQUIRE(ctx, "d2d_mov_sample: null argument");
  D2D_REQUIRE(G >= 1 && N >= 1 && h > 0, "d2d_mov_sample: G >= 1, N >= 1, h > 0 required (G=%d N=%d h=%g)", G, N, h);
  if (int rc = check_moving(mov, ctr, t_start, "d2d_mov_sample")) return rc;
  return nlp_mov_sample_launch(ctx, G, N, h, t_start, *mov, ctr);
}

int d2d_nlp_solve_moving(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W, double *work,
                         double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, const d2d_wind_field *f,
                         const double *t_start, const d2d_moving_obstacles *mov, double *mov_work) {
  if (int rc = nlp_single_check(ctx, B, N, h, scen, W, work, cost, feas, "d2d_nlp_solve_moving")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_moving_prologue(ctx, B, N, h, opts, f, t_start, mov, mov_work, "d2d_nlp_solve_moving", &o)) return rc;
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_handout_launch(nlp_solve_moving_kernel<decltype(wind)::value>, ctx, B, N, h, o, scen, W, work, mult, cost, feas, iters, status, wf,
                              t_start, *mov, (const double *)mov_work);
  });
}

int d2d_nlp_solve_keepout(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W, double *work,
                          double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, const d2d_wind_field *f,
                          const double *t_start, const d2d_keep_out *keep, double *kwork) {
  D2D_REQUIRE(keep, "d2d_nlp_solve_keepout: null keep-out table (n_keep = 0: no discs)");
  D2D_REQUIRE(keep->n_keep >= 0 && keep->n_keep <= D2D_MAX_KEEP, "d2d_nlp_solve_keepout: n_keep = %d outside 0 .. %d", keep->n_keep, D2D_MAX_KEEP);
  if (keep->n_keep == 0) {                                 // no discs: the solve of d2d_nlp_solve_moving with nothing moving, its kernels and its checks
    const d2d_moving_obstacles none{0, 0, nullptr, nullptr};
    return d2d_nlp_solve_moving(ctx, B, N, h, scen, opts, W, work, mult, cost, feas, iters, status, f, t_start, &none, nullptr);
  }
  if (int rc = nlp_single_check(ctx, B, N, h, scen, W, work, cost, feas, "d2d_nlp_solve_keepout")) return rc;
  D2D_REQUIRE(keep->discs && kwork, "d2d_nlp_solve_keepout: null discs or kwork with n_keep = %d", keep->n_keep);
  if (int rc = nlp_field_check(f, t_start, nullptr, "d2d_nlp_solve_keepout")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_keepout", &o)) return rc;
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_handout_launch(nlp_solve_keepout_kernel<decltype(wind)::value>, ctx, B, N, h, o, scen, W, work, mult, cost, feas, iters, status, wf,
                              t_start, *keep, kwork);
  });
}

int d2d_nlp_solve_fence(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W, double *work,
                        double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, const d2d_wind_field *f,
                        const double *t_start, const d2d_keep_out *keep, double *kwork, const d2d_fence *fence, double *fwork) {
  D2D_REQUIRE(fence, "d2d_nlp_solve_fence: null fence (n_edge = 0: no edges)");
  D2D_REQUIRE(fence->n_edge >= 0 && fence->n_edge <= D2D_MAX_FENCE, "d2d_nlp_solve_fence: n_edge = %d outside 0 .. %d", fence->n_edge, D2D_MAX_FENCE);
  if (fence->n_edge == 0)                                  // no edges: the solve of d2d_nlp_solve_keepout, its kernels and its checks
    return d2d_nlp_solve_keepout(ctx, B, N, h, scen, opts, W, work, mult, cost, feas, iters, status, f, t_start, keep, kwork);
  D2D_REQUIRE(fence->edges && fwork, "d2d_nlp_solve_fence: null edges or fwork with n_edge = %d", fence->n_edge);
  D2D_REQUIRE(keep, "d2d_nlp_solve_fence: null keep-out table (n_keep = 0: no discs)");
  D2D_REQUIRE(keep->n_keep >= 0 && keep->n_keep <= D2D_MAX_KEEP, "d2d_nlp_solve_fence: n_keep = %d outside 0 .. %d", keep->n_keep, D2D_MAX_KEEP);
  D2D_REQUIRE(keep->n_keep == 0 || (keep->discs && kwork), "d2d_nlp_solve_fence: null discs or kwork with n_keep = %d", keep->n_keep);
  if (int rc = nlp_single_check(ctx, B, N, h, scen, W, work, cost, feas, "d2d_nlp_solve_fence")) return rc;
  if (int rc = nlp_field_check(f, t_start, nullptr, "d2d_nlp_solve_fence")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_fence", &o)) return rc;
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_handout_launch(nlp_solve_fence_kernel<decltype(wind)::value>, ctx, B, N, h, o, scen, W, work, mult, cost, feas, iters, status, wf,
                              t_start, *keep, kwork, *fence, fwork);
  });
}

int d2d_nlp_solve_keepout_moving(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W, double *work,
                                 double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, const d2d_wind_field *f,
                                 const double *t_start, const d2d_moving_obstacles *mov, double *mov_work, double *kwork) {
  if (int rc = nlp_single_check(ctx, B, N, h, scen, W, work, cost, feas, "d2d_nlp_solve_keepout_moving")) return rc;
  D2D_REQUIRE(!mov || mov->n_mov == 0 || kwork, "d2d_nlp_solve_keepout_moving: null kwork with n_mov = %d", mov->n_mov);
  d2d_nlp_opts o;
  if (int rc = nlp_moving_prologue(ctx, B, N, h, opts, f, t_start, mov, mov_work, "d2d_nlp_solve_keepout_moving", &o)) return rc;
  if (mov->n_mov == 0)                                     // no discs: the solve of d2d_nlp_solve_moving with nothing moving
    return d2d_nlp_solve_moving(ctx, B, N, h, scen, opts, W, work, mult, cost, feas, iters, status, f, t_start, mov, mov_work);
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_handout_launch(nlp_solve_keepout_moving_kernel<decltype(wind)::value>, ctx, B, N, h, o, scen, W, work, mult, cost, feas, iters, status,
                              wf, t_start, *mov, (const double *)mov_work, kwork);
  });
}

int d2d_nlp_solve_groups_keepout(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                                 double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                                 int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start,
                                 const d2d_moving_obstacles *mov, double *mov_work, double *kwork) {
  if (int rc = nlp_groups_check(ctx, R, n_ac, N, h, scen, max_sweeps, tol, W, work, cost, feas, "d2d_nlp_solve_groups_keepout")) return rc;
  D2D_REQUIRE(!mov || mov->n_mov == 0 || kwork, "d2d_nlp_solve_groups_keepout: null kwork with n_mov = %d", mov->n_mov);
  d2d_nlp_opts o;
  if (int rc = nlp_moving_prologue(ctx, R, N, h, opts, f, t_start, mov, mov_work, "d2d_nlp_solve_groups_keepout", &o)) return rc;
  if (mov->n_mov == 0)                                     // no discs: the solve of d2d_nlp_solve_groups_pairs
    return d2d_nlp_solve_groups_pairs(ctx, R, n_ac, N, h, scen, opts, max_sweeps, tol, W, work, mult, cost, feas, iters, status, sweeps, moved, f,
                                      t_start);
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_groups_launch(nlp_groups_keepout_kernel<decltype(wind)::value>, ctx, R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult,
                             nlp_groups_prev(work, R, n_ac, N), cost, feas, iters, status, sweeps, moved, wf, t_start, *mov,
                             (const double *)mov_work, kwork);
  });
}

int d2d_nlp_solve_groups_fence(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                               double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                               int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start,
                               const d2d_fence *fence, double *fwork) {
  D2D_REQUIRE(fence, "d2d_nlp_solve_groups_fence: null fence (n_edge = 0: no edges)");
  D2D_REQUIRE(fence->n_edge >= 0 && fence->n_edge <= D2D_MAX_FENCE, "d2d_nlp_solve_groups_fence: n_edge = %d outside 0 .. %d", fence->n_edge,
              D2D_MAX_FENCE);
  if (fence->n_edge == 0)                                  // no edges: the solve of d2d_nlp_solve_groups_pairs
    return d2d_nlp_solve_groups_pairs(ctx, R, n_ac, N, h, scen, opts, max_sweeps, tol, W, work, mult, cost, feas, iters, status, sweeps, moved, f,
                                      t_start);
  D2D_REQUIRE(fence->edges && fwork, "d2d_nlp_solve_groups_fence: null edges or fwork with n_edge = %d", fence->n_edge);
  if (int rc = nlp_groups_check(ctx, R, n_ac, N, h, scen, max_sweeps, tol, W, work, cost, feas, "d2d_nlp_solve_groups_fence")) return rc;
  if (int rc = nlp_field_check(f, t_start, nullptr, "d2d_nlp_solve_groups_fence")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_options(opts, "d2d_nlp_solve_groups_fence", &o)) return rc;
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_groups_launch(nlp_groups_fence_kernel<decltype(wind)::value>, ctx, R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult,
                             nlp_groups_prev(work, R, n_ac, N), cost, feas, iters, status, sweeps, moved, wf, t_start, *fence, fwork);
  });
}

int d2d_nlp_solve_groups_moving(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                                double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                                int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start,
                                const d2d_moving_obstacles *mov, double *mov_work) {
  if (int rc = nlp_groups_check(ctx, R, n_ac, N, h, scen, max_sweeps, tol, W, work, cost, feas, "d2d_nlp_solve_groups_moving")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_moving_prologue(ctx, R, N, h, opts, f, t_start, mov, mov_work, "d2d_nlp_solve_groups_moving", &o)) return rc;
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_groups_launch(nlp_groups_moving_kernel<decltype(wind)::value>, ctx, R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult,
                             nlp_groups_prev(work, R, n_ac, N), cost, feas, iters, status, sweeps, moved, wf, t_start, *mov,
                             (const double *)mov_work);
  });
}

int d2d_nlp_solve_via(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_opts *opts, double *W, double *work,
                      double *mult, double *cost, double *feas, int32_t *iters, int32_t *status, const d2d_wind_field *f,
                      const double *t_start, const d2d_moving_obstacles *mov, double *mov_work, const d2d_via_points *via, int32_t *via_work) {
  const d2d_moving_obstacles none{0, 0, nullptr, nullptr};
  if (!mov) mov = &none;
  if (int rc = check_via(via, via_work, "d2d_nlp_solve_via")) return rc;
  if (via->n_via == 0)                                     // no pins: the solve of d2d_nlp_solve_moving, its kernels and its checks
    return d2d_nlp_solve_moving(ctx, B, N, h, scen, opts, W, work, mult, cost, feas, iters, status, f, t_start, mov, mov_work);
  if (int rc = nlp_single_check(ctx, B, N, h, scen, W, work, cost, feas, "d2d_nlp_solve_via")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_moving_prologue(ctx, B, N, h, opts, f, t_start, mov, mov_work, "d2d_nlp_solve_via", &o)) return rc;
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_handout_launch(nlp_solve_via_kernel<decltype(wind)::value>, ctx, B, N, h, o, scen, W, work, mult, cost, feas, iters, status, wf,
                              t_start, *mov, (const double *)mov_work, *via, via_work);
  });
}

int d2d_nlp_solve_groups_via(d2d_ctx *ctx, int R, int n_ac, int N, double h, const double *scen, const d2d_nlp_opts *opts, int max_sweeps,
                             double tol, double *W, double *work, double *mult, double *cost, double *feas, int32_t *iters,
                             int32_t *status, int32_t *sweeps, double *moved, const d2d_wind_field *f, const double *t_start,
                             const d2d_moving_obstacles *mov, double *mov_work, const d2d_via_points *via, int32_t *via_work) {
  const d2d_moving_obstacles none{0, 0, nullptr, nullptr};
  if (!mov) mov = &none;
  if (int rc = check_via(via, via_work, "d2d_nlp_solve_groups_via")) return rc;
  if (via->n_via == 0)                                     // no pins: the solve of d2d_nlp_solve_groups_moving, its kernels and its checks
    return d2d_nlp_solve_groups_moving(ctx, R, n_ac, N, h, scen, opts, max_sweeps, tol, W, work, mult, cost, feas, iters, status, sweeps, moved, f,
                                       t_start, mov, mov_work);
  if (int rc = nlp_groups_check(ctx, R, n_ac, N, h, scen, max_sweeps, tol, W, work, cost, feas, "d2d_nlp_solve_groups_via")) return rc;
  d2d_nlp_opts o;
  if (int rc = nlp_moving_prologue(ctx, R, N, h, opts, f, t_start, mov, mov_work, "d2d_nlp_solve_groups_via", &o)) return rc;
  return nlp_with_field(f, [&](auto wind, const d2d_wind_field &wf) {
    return nlp_groups_launch(nlp_groups_via_kernel<decltype(wind)::value>, ctx, R, n_ac, N, h, o, max_sweeps, tol, scen, W, work, mult,
                             nlp_groups_prev(work, R, n_ac, N), cost, feas, iters, status, sweeps, moved, wf, t_start, *mov,
                             (const double *)mov_work, *via, via_work);
  });
}

}  // extern "C"
