// d2d_flight_audit: one streaming pass over a state history [n_rows][5][N] that is already on the device -- closest approach between
// the aircraft of a formation (continuous in time between rows), clearance from static and moving discs, tracking error, bank and
// airspeed envelope (include/d2d.h; tests/flight_audit_ref.py is the CPU statement).
//
// Three kernels.  audit_check_kernel: a lane per formation checks the start time and the tracks.  audit_partial_kernel: lanes along the drone index (a wave reads 512 contiguous bytes per plane row), a workgroup owns
// whole formations, the rows are cut into blocks of rows_per_block and every (workgroup, row block) keeps, per lane, its minima,
// maxima and counts, which it stores as one partial per block.  audit_combine_kernel: a lane per drone folds the partials in ascending
// block order and writes the outputs.  Every candidate is a key (squared distance, row index + s, partner) that is computed in ONE
// place from values that do not depend on the block length (the row index is the history's, not the block's), and the fold is the
// lexicographic minimum of those keys -- associative and commutative -- so the outputs are bit-identical for every block length.
// No floating-point atomic, no sum.
//
// A segment's candidates: the row itself (s = 0, q = p0; computed by the block that owns the row), and the interior minimum where
// 0 < s* < 1.  s* = 1 is the next row's own candidate (q = p1 exactly, at the same time), so nothing is computed twice and the
// segment that joins two blocks is audited once, by the block that owns its first row (it reads one row past its end).
//
// The work of a row block is split into tasks, the fastest-varying part of the workgroup index: task 0 is the separation (partners
// through LDS), the tracking error and the envelope; task k >= 1 is the clearance from discs 4 (k - 1) .. 4 k - 1 of the list
// (static discs, then moving discs), which re-reads the x and y planes (its neighbour in the launch has just fetched them).
#include "common.h"
#include "audit_device.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

namespace {

constexpr int AUD_WG = 256;          // lanes of a workgroup: floor(256 / n_ac) whole formations
constexpr int AUD_DISCS = 4;         // discs of a clearance task (their accumulators stay in registers)
constexpr int AUD_MIN_RPB = 16;      // the library's block length is at least this (a block reads one row more than it owns)
constexpr int AUD_WAVES = 8192;      // ... and is chosen so that the launch has about this many wavefronts
// status bits of a refused formation (include/d2d.h D2D_AUDIT_*)
constexpr int AUD_BAD_VALUE = D2D_AUDIT_NONFINITE, AUD_BAD_TSTART = D2D_AUDIT_BAD_TSTART, AUD_BAD_TRACK = D2D_AUDIT_BAD_TRACK;

// double / int32 planes [N] of a row block's partial
enum { PD_SEP_D2, PD_SEP_U, PD_ERR_E2, PD_ERR_U, PD_PHI, PD_VMIN, PD_VMAX, PD_DISC };   // disc k: PD_DISC + 2 k (d2), + 1 (u)
enum { PI_SEP_J, PI_SEP_CNT, PI_ERR_CNT, PI_DISC };                                     // disc k: PI_DISC + k (count)

struct AuditArgs {
  d2d_audit_params p;
  int n_mov, n_wgx, n_task, nb, rpb, N;
  const double *X, *t_start, *x_ref, *y_ref, *stat, *mov_disc, *mov_ctr;
  const int32_t *rows;
  int32_t *fbad;
  double *pd;
  int32_t *pi;
  d2d_audit_out out;
  unsigned want;                     // WANT_* of the requested outputs
};
enum : unsigned { WANT_SEP = 1, WANT_ERR = 2, WANT_PHI = 4, WANT_V = 8, WANT_STAT = 16, WANT_MOV = 32 };

__device__ __forceinline__ const double *aud_plane(const double *X, int N, int row, int plane) {
  return X + ((size_t)row * 5 + plane) * (size_t)N;
}

// task 0 of a row block: separation, tracking error, envelope.  Called by every lane of the workgroup (barriers inside).
__device__ __forceinline__ void aud_core(const AuditArgs &A, int d, bool active, int f, int rows_f, int i0, int i1, int b,
                                         double (*lx)[AUD_WG], double (*ly)[AUD_WG]) {
  const int N = A.N, n_ac = A.p.n_ac, tid = threadIdx.x;
  const bool want_sep = (A.want & WANT_SEP) && n_ac > 1, want_err = A.want & WANT_ERR, want_phi = A.want & WANT_PHI, want_v = A.want & WANT_V;
  const bool want_xy = (A.want & WANT_SEP) || want_err;     // (n_ac = 1: no partner, x and y are still checked)
  const int a = active ? d % n_ac : 0, lbase = tid - a;
  const double safe2 = A.p.d_safe > 0.0 ? A.p.d_safe * A.p.d_safe : 0.0, tol2 = A.p.err_tol * A.p.err_tol;
  double sd2 = aud_inf(), su = aud_nan(); int sj = -1, scnt = 0;
  double e2max = -aud_inf(), eu = aud_nan(); int ecnt = 0;
  double phimax = -aud_inf(), vmin = aud_inf(), vmax = -aud_inf();
  int bad = 0;
  // rows i (c), i + 1 (n) and the prefetched i + 2 (q) of the lane's own planes; x, y of a row past the block's end only for the segment
  double cx = 0, cy = 0, nx = 0, ny = 0, qx = 0, qy = 0;
  double cphi = 0, cv = 0, cxr = 0, cyr = 0, nphi = 0, nv = 0, nxr = 0, nyr = 0;
  auto load_xy = [&](int r, double &x, double &y) {
    if (want_xy && r < rows_f && r <= i1) { x = aud_plane(A.X, N, r, 0)[d]; y = aud_plane(A.X, N, r, 1)[d]; }
  };
  auto load_row = [&](int r, double &phi, double &v, double &xr, double &yr) {
    if (r < rows_f && r < i1) {
      if (want_phi) phi = aud_plane(A.X, N, r, 3)[d];
      if (want_v) v = aud_plane(A.X, N, r, 4)[d];
      if (want_err) { xr = A.x_ref[(size_t)r * N + d]; yr = A.y_ref[(size_t)r * N + d]; }
    }
  };
  load_xy(i0, cx, cy); load_row(i0, cphi, cv, cxr, cyr);
  load_xy(i0 + 1, nx, ny); load_row(i0 + 1, nphi, nv, nxr, nyr);
  if (want_sep) { lx[i0 % 3][tid] = cx; ly[i0 % 3][tid] = cy; }
  for (int i = i0; i < i1; ++i) {
    double qphi = 0, qv = 0, qxr = 0, qyr = 0;
    load_xy(i + 2, qx, qy); load_row(i + 2, qphi, qv, qxr, qyr);
    const bool row = i < rows_f, seg = i + 1 < rows_f;
    if (want_sep) {
      lx[(i + 1) % 3][tid] = nx; ly[(i + 1) % 3][tid] = ny;
      __syncthreads();               // three buffers: a wave that writes row i + 2 has passed this barrier, behind every read of row i - 1
      if (row) {
        const double *x0 = lx[i % 3] + lbase, *y0 = ly[i % 3] + lbase, *x1 = lx[(i + 1) % 3] + lbase, *y1 = ly[(i + 1) % 3] + lbase;
        double rmin = aud_inf();
        for (int j = 0; j < n_ac; ++j) {
          if (j == a) continue;
          const double r2 = aud_segment(x0[j] - cx, y0[j] - cy, x1[j] - nx, y1[j] - ny, seg, i, j, sd2, su, sj);
          rmin = fmin(rmin, r2);
        }
        scnt += rmin < safe2;
      }
    }
    if (row) {
      if (want_xy) bad |= !aud_finite(cx) || !aud_finite(cy);
      if (want_err) {
        const double ex = cx - cxr, ey = cy - cyr, e2 = fma(ex, ex, ey * ey);
        bad |= !aud_finite(cxr) || !aud_finite(cyr);
        if (e2 > e2max) { e2max = e2; eu = (double)i; }
        ecnt += e2 > tol2;
      }
      if (want_phi) { bad |= !aud_finite(cphi); phimax = fmax(phimax, fabs(cphi)); }
      if (want_v) { bad |= !aud_finite(cv); vmin = fmin(vmin, cv); vmax = fmax(vmax, cv); }
    }
    cx = nx; cy = ny; nx = qx; ny = qy;
    cphi = nphi; cv = nv; cxr = nxr; cyr = nyr; nphi = qphi; nv = qv; nxr = qxr; nyr = qyr;
  }
  if (!active) return;
  if (bad) atomicOr(A.fbad + f, AUD_BAD_VALUE);
  double *pd = A.pd + (size_t)b * (PD_DISC + 2 * (A.p.n_stat + A.n_mov)) * N + d;
  int32_t *pi = A.pi + (size_t)b * (PI_DISC + A.p.n_stat + A.n_mov) * N + d;
  if (want_sep) {
    pd[(size_t)PD_SEP_D2 * N] = sd2; pd[(size_t)PD_SEP_U * N] = su; pi[(size_t)PI_SEP_J * N] = sj; pi[(size_t)PI_SEP_CNT * N] = scnt;
  }
  if (want_err) { pd[(size_t)PD_ERR_E2 * N] = e2max; pd[(size_t)PD_ERR_U * N] = eu; pi[(size_t)PI_ERR_CNT * N] = ecnt; }
  if (want_phi) pd[(size_t)PD_PHI * N] = phimax;
  if (want_v) { pd[(size_t)PD_VMIN * N] = vmin; pd[(size_t)PD_VMAX * N] = vmax; }
}

// task k >= 1 of a row block: the clearance from discs k0 .. k0 + 3 of the list (static, then moving).  No barrier inside.
__device__ __forceinline__ void aud_discs(const AuditArgs &A, int d, int f, int rows_f, int i0, int i1, int b, int k0) {
  const int N = A.N, n_stat = A.p.n_stat, n_disc = n_stat + A.n_mov, n_rows = A.p.n_rows;
  double bd2[AUD_DISCS], bu[AUD_DISCS], r2lim[AUD_DISCS], c0x[AUD_DISCS], c0y[AUD_DISCS], c1x[AUD_DISCS], c1y[AUD_DISCS];
  int cnt[AUD_DISCS];
  const double *mx[AUD_DISCS];       // a moving disc's x centres at the rows (y: + n_rows), NULL for a static disc
  bool on[AUD_DISCS];
  int bad = 0;
#pragma unroll
  for (int k = 0; k < AUD_DISCS; ++k) {
    const int disc = k0 + k;
    bd2[k] = aud_inf(); bu[k] = aud_nan(); cnt[k] = 0; mx[k] = nullptr; on[k] = false;
    r2lim[k] = c0x[k] = c0y[k] = c1x[k] = c1y[k] = 0.0;
    if (disc < n_stat) {
      if (A.want & WANT_STAT) {
        const double *t = A.stat + ((size_t)f * n_stat + disc) * 3;
        const double r = t[2];
        on[k] = !(r <= 0.0);
        if (on[k]) {
          c0x[k] = c1x[k] = t[0]; c0y[k] = c1y[k] = t[1]; r2lim[k] = r * r;
          bad |= !aud_finite(t[0]) || !aud_finite(t[1]) || !aud_finite(r);
        }
      }
    } else if (disc < n_disc && (A.want & WANT_MOV)) {
      const int m = disc - n_stat;
      const double r = A.mov_disc[((size_t)f * A.n_mov + m) * 2];
      on[k] = !(r <= 0.0);
      if (on[k]) {
        r2lim[k] = r * r;
        bad |= !aud_finite(r);
        mx[k] = A.mov_ctr + ((size_t)f * A.n_mov + m) * 2 * (size_t)n_rows;
        if (i0 < rows_f) { c0x[k] = mx[k][i0]; c0y[k] = mx[k][n_rows + i0]; }
      }
    }
  }
  double cx = 0, cy = 0, nx = 0, ny = 0, qx = 0, qy = 0;
  auto load_xy = [&](int r, double &x, double &y) {
    if (r < rows_f && r <= i1) { x = aud_plane(A.X, N, r, 0)[d]; y = aud_plane(A.X, N, r, 1)[d]; }
  };
  load_xy(i0, cx, cy); load_xy(i0 + 1, nx, ny);
  for (int i = i0; i < i1 && i < rows_f; ++i) {
    load_xy(i + 2, qx, qy);
    const bool seg = i + 1 < rows_f;
    bad |= !aud_finite(cx) || !aud_finite(cy);
#pragma unroll
    for (int k = 0; k < AUD_DISCS; ++k) {
      if (!on[k]) continue;
      if (mx[k] && seg) { c1x[k] = mx[k][i + 1]; c1y[k] = mx[k][n_rows + i + 1]; }
      int none = 0;
      const double r2 = aud_segment(cx - c0x[k], cy - c0y[k], nx - c1x[k], ny - c1y[k], seg, i, 0, bd2[k], bu[k], none);
      cnt[k] += r2 < r2lim[k];
      c0x[k] = c1x[k]; c0y[k] = c1y[k];
    }
    cx = nx; cy = ny; nx = qx; ny = qy;
  }
  if (bad) atomicOr(A.fbad + f, AUD_BAD_VALUE);
  double *pd = A.pd + (size_t)b * (PD_DISC + 2 * n_disc) * N + d;
  int32_t *pi = A.pi + (size_t)b * (PI_DISC + n_disc) * N + d;
#pragma unroll
  for (int k = 0; k < AUD_DISCS; ++k) {
    const int disc = k0 + k;
    if (disc < n_disc && (A.want & (disc < n_stat ? WANT_STAT : WANT_MOV))) {
      pd[(size_t)(PD_DISC + 2 * disc) * N] = bd2[k]; pd[(size_t)(PD_DISC + 2 * disc + 1) * N] = bu[k]; pi[(size_t)(PI_DISC + disc) * N] = cnt[k];
    }
  }
}

__global__ void __launch_bounds__(AUD_WG)
audit_partial_kernel(AuditArgs A) {
  __shared__ double lx[3][AUD_WG], ly[3][AUD_WG];
  __shared__ int wg_rows;
  const int task = blockIdx.x % A.n_task;
  const int rest = blockIdx.x / A.n_task, wgx = rest % A.n_wgx, b = rest / A.n_wgx;
  const int n_ac = A.p.n_ac, dpw = (AUD_WG / n_ac) * n_ac, tid = threadIdx.x;
  const int d = wgx * dpw + tid;
  const bool active = tid < dpw && d < A.N;
  const int f = active ? d / n_ac : 0;
  int rows_f = 0;
  if (active) rows_f = A.rows ? min(max(A.rows[f], 0), A.p.n_rows) : A.p.n_rows;
  const int i0 = b * A.rpb;
  int i1 = min(i0 + A.rpb, A.p.n_rows);
  if (task == 0) {
    if (tid == 0) wg_rows = 0;
    __syncthreads();
    atomicMax(&wg_rows, rows_f);
    __syncthreads();
    i1 = min(i1, wg_rows);           // rows that no formation of the workgroup holds: nothing to do, the same for every lane
    aud_core(A, d, active, f, rows_f, i0, i1, b, lx, ly);
  } else if (active) {
    aud_discs(A, d, f, rows_f, i0, i1, b, (task - 1) * AUD_DISCS);
  }
}

// The tracks of formation f by the rules of d2d_nlp_solve_moving: a non-finite knot, times that do not increase strictly, a kind that
// is neither 0 nor 1 (absent discs included).
__device__ __forceinline__ bool aud_track_bad(const AuditArgs &A, const d2d_moving_obstacles &mv, int f) {
  bool bad = false;
  const double *kn = mv.knots + (size_t)f * mv.n_mov * mv.n_knot * 3;
  for (int e = 0; e < mv.n_mov * mv.n_knot; ++e) {
    const double t = kn[3 * e];
    bad |= !aud_finite(t) || !aud_finite(kn[3 * e + 1]) || !aud_finite(kn[3 * e + 2]);
    if (e % mv.n_knot != 0) bad |= !(t > kn[3 * (e - 1)]);
  }
  for (int m = 0; m < mv.n_mov; ++m) {
    const double kind = mv.disc[((size_t)f * mv.n_mov + m) * 2 + 1];
    bad |= !(kind == 0.0 || kind == 1.0);
  }
  return bad;
}

// a lane per formation, ahead of the partial kernel (which ORs its own bit into the same word): the start time and the tracks
__global__ void __launch_bounds__(AUD_WG)
audit_check_kernel(AuditArgs A, d2d_moving_obstacles mv) {
  const int f = blockIdx.x * AUD_WG + threadIdx.x;
  if (f >= A.p.n_form) return;
  int status = 0;
  if (A.t_start && !aud_finite(A.t_start[f])) status |= AUD_BAD_TSTART;
  if (A.n_mov > 0 && aud_track_bad(A, mv, f)) status |= AUD_BAD_TRACK;
  if (status) atomicOr(A.fbad + f, status);
}

__global__ void __launch_bounds__(AUD_WG)
audit_combine_kernel(AuditArgs A) {
  const int d = blockIdx.x * AUD_WG + threadIdx.x, N = A.N;
  if (d >= N) return;
  const int n_ac = A.p.n_ac, f = d / n_ac, n_stat = A.p.n_stat, n_disc = n_stat + A.n_mov;
  const double t0 = A.t_start ? A.t_start[f] : 0.0, dt = A.p.dt_row;
  const int status = A.fbad[f];
  if (A.out.status && d % n_ac == 0) A.out.status[f] = status;
  const bool ok = status == 0;
  const double nan = aud_nan();
  const size_t sd = (size_t)(PD_DISC + 2 * n_disc) * N, si = (size_t)(PI_DISC + n_disc) * N;
  const double *pd = A.pd + d;
  const int32_t *pi = A.pi + d;
  auto when = [&](double u) { return fma(u, dt, t0); };     // NaN (nothing seen) stays NaN
  if (A.want & WANT_SEP) {
    double bd2 = aud_inf(), bu = nan; int bj = -1, cnt = 0;
    if (ok && n_ac > 1)
      for (int b = 0; b < A.nb; ++b) {
        const double d2 = pd[b * sd + (size_t)PD_SEP_D2 * N], u = pd[b * sd + (size_t)PD_SEP_U * N];
        const int j = pi[b * si + (size_t)PI_SEP_J * N];
        cnt += pi[b * si + (size_t)PI_SEP_CNT * N];
        if (j >= 0 && (bj < 0 || aud_less(d2, u, j, bd2, bu, bj))) { bd2 = d2; bu = u; bj = j; }
      }
    if (A.out.sep_dist) A.out.sep_dist[d] = ok ? sqrt(bd2) : nan;
    if (A.out.sep_time) A.out.sep_time[d] = ok ? when(bu) : nan;
    if (A.out.sep_partner) A.out.sep_partner[d] = ok ? bj : -1;
    if (A.out.sep_count) A.out.sep_count[d] = ok ? cnt : -1;
  }
  for (int disc = 0; disc < n_disc; ++disc) {
    const bool stat = disc < n_stat;
    if (!(A.want & (stat ? WANT_STAT : WANT_MOV))) continue;
    const double r = stat ? A.stat[((size_t)f * n_stat + disc) * 3 + 2] : A.mov_disc[((size_t)f * A.n_mov + (disc - n_stat)) * 2];
    double bd2 = aud_inf(), bu = nan; int cnt = 0;
    if (ok && !(r <= 0.0))
      for (int b = 0; b < A.nb; ++b) {
        const double d2 = pd[b * sd + (size_t)(PD_DISC + 2 * disc) * N], u = pd[b * sd + (size_t)(PD_DISC + 2 * disc + 1) * N];
        cnt += pi[b * si + (size_t)(PI_DISC + disc) * N];
        if (u == u && (bu != bu || aud_less(d2, u, 0, bd2, bu, 0))) { bd2 = d2; bu = u; }
      }
    const size_t o = (size_t)(stat ? disc : disc - n_stat) * N + d;
    double *clear = stat ? A.out.stat_clear : A.out.mov_clear, *time = stat ? A.out.stat_time : A.out.mov_time;
    int32_t *count = stat ? A.out.stat_count : A.out.mov_count;
    if (clear) clear[o] = ok ? (bu == bu ? sqrt(bd2) - r : aud_inf()) : nan;
    if (time) time[o] = ok ? when(bu) : nan;
    if (count) count[o] = ok ? cnt : -1;
  }
  if (A.want & WANT_ERR) {
    double e2 = -aud_inf(), eu = nan; int cnt = 0;
    if (ok)
      for (int b = 0; b < A.nb; ++b) {
        const double v = pd[b * sd + (size_t)PD_ERR_E2 * N], u = pd[b * sd + (size_t)PD_ERR_U * N];
        cnt += pi[b * si + (size_t)PI_ERR_CNT * N];
        if (v > e2) { e2 = v; eu = u; }          // ascending blocks: the earliest row of the largest error
      }
    if (A.out.err_max) A.out.err_max[d] = ok ? (eu == eu ? sqrt(e2) : -aud_inf()) : nan;
    if (A.out.err_time) A.out.err_time[d] = ok ? when(eu) : nan;
    if (A.out.err_count) A.out.err_count[d] = ok ? cnt : -1;
  }
  if (A.want & WANT_PHI) {
    double v = -aud_inf();
    if (ok) for (int b = 0; b < A.nb; ++b) v = fmax(v, pd[b * sd + (size_t)PD_PHI * N]);
    A.out.phi_max[d] = ok ? v : nan;
  }
  if (A.want & WANT_V) {
    double lo = aud_inf(), hi = -aud_inf();
    if (ok) for (int b = 0; b < A.nb; ++b) { lo = fmin(lo, pd[b * sd + (size_t)PD_VMIN * N]); hi = fmax(hi, pd[b * sd + (size_t)PD_VMAX * N]); }
    if (A.out.v_min) A.out.v_min[d] = ok ? lo : nan;
    if (A.out.v_max) A.out.v_max[d] = ok ? hi : nan;
  }
}

// what makes the arguments D2D_EINVAL (include/d2d.h), and the launch geometry they give
int audit_plan(const d2d_audit_params *p, int n_mov, const char *who, AuditArgs &A) {
  D2D_REQUIRE(p, "%s: null parameters", who);
  D2D_REQUIRE(p->n_form >= 1 && p->n_ac >= 1 && p->n_ac <= 64, "%s: n_form >= 1 and n_ac in 1 .. 64 required (n_form=%d n_ac=%d)", who, p->n_form, p->n_ac);
  D2D_REQUIRE(p->n_rows >= 1 && p->dt_row > 0, "%s: n_rows >= 1 and dt_row > 0 required (n_rows=%d dt_row=%g)", who, p->n_rows, p->dt_row);
  D2D_REQUIRE(p->n_stat >= 0 && p->n_stat <= D2D_MAX_OBS, "%s: n_stat = %d outside 0 .. %d", who, p->n_stat, D2D_MAX_OBS);
  D2D_REQUIRE(n_mov >= 0 && n_mov <= D2D_MAX_MOV, "%s: n_mov = %d outside 0 .. %d", who, n_mov, D2D_MAX_MOV);
  D2D_REQUIRE(p->rows_per_block >= 0, "%s: rows_per_block = %d (0: the library's choice)", who, p->rows_per_block);
  D2D_REQUIRE(!(p->err_tol != p->err_tol) && p->err_tol >= 0, "%s: err_tol must be >= 0", who);
  const long long N = (long long)p->n_form * p->n_ac;
  D2D_REQUIRE(N * 5 * (long long)p->n_rows < (1LL << 40) && N < (1LL << 31), "%s: history too large", who);
  A.p = *p; A.n_mov = n_mov; A.N = (int)N;
  const int fpw = AUD_WG / p->n_ac;
  A.n_wgx = (p->n_form + fpw - 1) / fpw;
  A.n_task = 1 + (p->n_stat + n_mov + AUD_DISCS - 1) / AUD_DISCS;
  int rpb = p->rows_per_block;
  if (rpb == 0) {
    const long long waves = (long long)A.n_wgx * (AUD_WG / 64) * A.n_task;
    const int nb = (int)std::max(1LL, (AUD_WAVES + waves - 1) / waves);
    rpb = std::max(AUD_MIN_RPB, (p->n_rows + nb - 1) / nb);
  }
  A.rpb = std::min(rpb, p->n_rows);
  A.nb = (p->n_rows + A.rpb - 1) / A.rpb;
  // (HIP refuses a launch of more than 2^32 lanes: 2^24 workgroups of 256)
  D2D_REQUIRE((long long)A.n_wgx * A.n_task * A.nb < (1LL << 24), "%s: more than 2^24 workgroups (rows_per_block = %d: use longer blocks)", who, p->rows_per_block);
  return D2D_OK;
}

size_t audit_fbad_bytes(const AuditArgs &A) { return ((size_t)A.p.n_form * sizeof(int32_t) + 15) / 16 * 16; }
size_t audit_pd_bytes(const AuditArgs &A) { return (size_t)A.nb * (PD_DISC + 2 * (A.p.n_stat + A.n_mov)) * A.N * sizeof(double); }
size_t audit_pi_bytes(const AuditArgs &A) { return (size_t)A.nb * (PI_DISC + A.p.n_stat + A.n_mov) * A.N * sizeof(int32_t); }

}  // namespace

extern "C" {

int64_t d2d_flight_audit_workspace(const d2d_audit_params *p, int n_mov) {
  AuditArgs A{};
  if (audit_plan(p, n_mov, "d2d_flight_audit_workspace", A)) return D2D_EINVAL;
  return (int64_t)(audit_fbad_bytes(A) + audit_pd_bytes(A) + audit_pi_bytes(A));
}

int d2d_flight_audit(d2d_ctx *ctx, const d2d_audit_params *p, const double *X_hist, const int32_t *rows, const double *t_start,
                     const double *x_ref, const double *y_ref, const double *stat, const d2d_moving_obstacles *mov, double *mov_work,
                     void *work, const d2d_audit_out *out) {
  D2D_REQUIRE(ctx && X_hist && out && work, "d2d_flight_audit: null argument (ctx, X_hist, work or out)");
  const int n_mov = mov ? mov->n_mov : 0;
  AuditArgs A{};
  if (int rc = audit_plan(p, n_mov, "d2d_flight_audit", A)) return rc;
  D2D_REQUIRE(p->n_stat == 0 || stat, "d2d_flight_audit: null table of static discs with n_stat = %d", p->n_stat);
  D2D_REQUIRE((x_ref != nullptr) == (y_ref != nullptr), "d2d_flight_audit: x_ref and y_ref go together");
  d2d_moving_obstacles mv{0, 0, nullptr, nullptr};
  if (n_mov > 0) {
    D2D_REQUIRE(mov->n_knot >= 2 && mov->n_knot <= D2D_MOV_MAX_KNOT, "d2d_flight_audit: n_knot = %d outside 2 .. %d", mov->n_knot, D2D_MOV_MAX_KNOT);
    D2D_REQUIRE(mov->knots && mov->disc, "d2d_flight_audit: null knots or disc table with n_mov = %d", n_mov);
    D2D_REQUIRE(mov_work, "d2d_flight_audit: null array of centre planes with n_mov = %d", n_mov);
    D2D_REQUIRE(t_start, "d2d_flight_audit: null t_start with n_mov = %d (a device array: the tracks' times are absolute)", n_mov);
    mv = *mov;
  }
  const d2d_audit_out &o = *out;
  A.out = o;
  A.want = (o.sep_dist || o.sep_partner || o.sep_time || o.sep_count ? WANT_SEP : 0u)
         | (x_ref && (o.err_max || o.err_time || o.err_count) ? WANT_ERR : 0u) | (o.phi_max ? WANT_PHI : 0u) | (o.v_min || o.v_max ? WANT_V : 0u)
         | (p->n_stat > 0 && (o.stat_clear || o.stat_time || o.stat_count) ? WANT_STAT : 0u)
         | (n_mov > 0 && (o.mov_clear || o.mov_time || o.mov_count) ? WANT_MOV : 0u);
  D2D_REQUIRE(x_ref || !(o.err_max || o.err_time || o.err_count), "d2d_flight_audit: tracking-error outputs without x_ref and y_ref");
  A.X = X_hist; A.rows = rows; A.t_start = t_start; A.x_ref = x_ref; A.y_ref = y_ref; A.stat = stat;
  A.mov_disc = mv.disc; A.mov_ctr = mov_work;
  char *w = static_cast<char *>(work);
  A.fbad = reinterpret_cast<int32_t *>(w);
  A.pd = reinterpret_cast<double *>(w + audit_fbad_bytes(A));
  A.pi = reinterpret_cast<int32_t *>(w + audit_fbad_bytes(A) + audit_pd_bytes(A));
  if (A.want & WANT_MOV)             // the centres at the row times: d2d_mov_sample's own kernel, so bit for bit its values
    if (int rc = d2d_mov_sample(ctx, p->n_form, p->n_rows, p->dt_row, t_start, &mv, mov_work)) return rc;
  D2D_CHECK_HIP(hipMemsetAsync(A.fbad, 0, audit_fbad_bytes(A), ctx->stream));
  hipLaunchKernelGGL(audit_check_kernel, dim3((unsigned)((p->n_form + AUD_WG - 1) / AUD_WG)), dim3(AUD_WG), 0, ctx->stream, A, mv);
  D2D_LAUNCH_CHECK();
  hipLaunchKernelGGL(audit_partial_kernel, dim3((unsigned)(A.n_wgx * A.n_task * A.nb)), dim3(AUD_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  hipLaunchKernelGGL(audit_combine_kernel, dim3((unsigned)((A.N + AUD_WG - 1) / AUD_WG)), dim3(AUD_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  return D2D_OK;
}

}  // extern "C"
