// d2d_wind_fit: the control points of a d2d_wind_field fitted to a state history [n_rows][5][N] that is already on the device
// (include/d2d.h states the estimator; tests/wind_fit_ref.py is the CPU statement, fixed-point rule included).
//
// Five kernels.
//   wf_accum_kernel    the hot path: A^T A and A^T m over (n_rows - 1) N samples.  A unit is D2D_WINDFIT_CHUNK = 64 consecutive samples
//                      of one drone; a workgroup of four wavefronts owns a contiguous range of (four drones, chunk) pairs, wavefront w the w-th drone
//                      of the four (a drone's units follow each other: time order; the four share their cache lines).  Lane
//                      r computes sample r of the unit (ten loads, cos / sin, the axis weights, the rejection); the accepted samples
//                      are then broadcast one by one and every lane adds ITS entries of the cell-local Gram w w^T: unsteady, lane j owns
//                      column j (64 sums); steady, lane (g, j) owns rows 4 g .. 4 g + 3 of column j (4 sums: the steady case never forms
//                      64 weights).  Every product is rounded to 2^-32 once and summed as a 64-bit integer, so the sums do not depend
//                      on where a wavefront hands them over: it keeps them in registers while the cell stays the same -- a drone moves
//                      under a metre per row, and the drones of a formation share cells -- and adds them to the stencil storage with
//                      integer atomics when the cell changes and at the end of its range.  No floating-point atomic, no float sum.
//   wf_convert_kernel  the integer sums back to fp64 (H_out, b_out, support), the penalties and mu folded into the system matrix.
//   wf_cg_kernel       one workgroup: Jacobi-preconditioned CG on both right-hand sides, the iterate staged in LDS, a wavefront per four
//                      matrix rows, reductions in a fixed order; writes cp_out and the counts.
//   wf_resid_kernel    the second streaming pass: the fitted field at the used samples, a fixed number of workgroups, one partial each.
//   wf_fold_kernel     folds the partials in ascending order.
//
// In registers the rounded products are summed as doubles: each is an integer of at most 2^32, so up to 2^20 of them add without
// rounding (the sum stays below 2^53) -- integer arithmetic at the fp64 rate; a wavefront hands over after 2^20 samples at the latest.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int WF_WG = 256;                    // lanes of an accumulation / residual workgroup: four wavefronts
constexpr int WF_WPB = WF_WG / 64;
constexpr int WF_CHUNK = D2D_WINDFIT_CHUNK;
static_assert(WF_CHUNK == 64, "a unit is one wavefront-load of samples");
constexpr int WF_WAVES = 8192;                // the library's choice of wavefronts for a large history
constexpr int WF_RES_BLOCKS = 256;            // workgroups of the residual pass: fixed, so its partials and their fold are too
constexpr int WF_CG_WG = 512;                  // one workgroup, two wavefronts a SIMD: 256 registers a lane for the rows in flight
constexpr double WF_SCALE = 4294967296.0;             // 2^32
enum { WF_OK = 0, WF_NONFINITE = 1, WF_OUTSIDE = 2, WF_OVER = 3 };

struct FitArgs {
  d2d_windfit_params p;
  d2d_wind_field g;                  // the geometry; cp: the prior or null
  int N, n_chunk, kt, nst, ncp, n_waves;
  long long n_units;
  double wp, inv_wp;                 // w_max rounded up to a power of two
  const double *X, *t_start;
  const int32_t *rows;
  unsigned long long *Hq, *bq, *cnt; // [ncp][nst], [2][ncp], [4]
  double *M, *rhs, *vec, *part;      // [ncp][nst], [2][ncp], CG vectors 4 x [2][ncp] + [ncp], [WF_RES_BLOCKS][2]
  int32_t *idx;                      // [ncp][nst]: the partner's index, -1 outside the grid
  double *cp_out;
  d2d_windfit_out out;
};

__device__ __forceinline__ bool wf_finite(double v) { return fabs(v) <= 1.79e308; }

// cos and sin by a fixed sequence of IEEE operations (include/d2d.h): the CPU statement repeats it operation for operation.
__device__ __forceinline__ void wf_sincos(double a, double &c, double &s) {
#pragma clang fp contract(off)
  const double k = rint(a * 6.36619772367581382433e-01);
  const double r = ((a - k * 1.57079632673412561417e+00) - k * 6.07710050630396597660e-11) - k * 2.02226624879595063154e-21;
  const double z = r * r;
  const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04
                  + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
  const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05
                  + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
  const double sr = r + (r * z) * ps;
  const double cr = 1.0 - (0.5 * z - (z * z) * pc);
  const int n = (int)((long long)k & 3);
  c = n == 0 ? cr : n == 1 ? -sr : n == 2 ? -cr : sr;
  s = n == 0 ? sr : n == 1 ? cr : n == 2 ? -sr : -cr;
}

// One axis: inside the box?  The segment and the four weights of wind_axis (wind_device.h), without contraction.
__device__ __forceinline__ bool wf_axis(double u, double u0, double h, int n, int &seg, double (&b)[4]) {
#pragma clang fp contract(off)
  const double s = (u - u0) / h;
  const bool in = s >= 0.0 && s <= (double)(n - 3);
  const double fl = in ? fmin(floor(s), (double)(n - 4)) : 0.0;
  const double r = in ? s - fl : 0.0, q = 1.0 - r, r2 = r * r, r3 = r2 * r;
  b[0] = q * q * q * (1.0 / 6.0);
  b[1] = (3.0 * r3 - 6.0 * r2 + 4.0) * (1.0 / 6.0);
  b[2] = (-3.0 * r3 + 3.0 * r2 + 3.0 * r + 1.0) * (1.0 / 6.0);
  b[3] = r3 * (1.0 / 6.0);
  seg = (int)fl;
  return in;
}

struct WfSample {
  double bx[4], by[4], bt[4], mx, my;
  int cell, why;                     // cell: the index of the cell's first control point
};

// Sample i (rows i, i + 1, both valid) of drone d in formation f.
__device__ __forceinline__ void wf_sample(const FitArgs &A, int d, int f, int i, WfSample &S) {
#pragma clang fp contract(off)
  const size_t N = (size_t)A.N;
  const double *r0 = A.X + (size_t)i * 5 * N + d, *r1 = r0 + 5 * N;
  const double x0 = r0[0], y0 = r0[N], a0 = r0[2 * N], f0 = r0[3 * N], v0 = r0[4 * N];
  const double x1 = r1[0], y1 = r1[N], a1 = r1[2 * N], f1 = r1[3 * N], v1 = r1[4 * N];
  const double dt = A.p.dt_row;
  const double tm = (A.t_start ? A.t_start[f] : 0.0) + ((double)i + 0.5) * dt;
  bool fin = wf_finite(x0) && wf_finite(y0) && wf_finite(a0) && wf_finite(f0) && wf_finite(v0)
          && wf_finite(x1) && wf_finite(y1) && wf_finite(a1) && wf_finite(f1) && wf_finite(v1);
  if (A.kt > 1) fin = fin && wf_finite(tm);
  int ix, iy, it = 0;
  bool in = wf_axis(0.5 * (x0 + x1), A.g.x0, A.g.hx, A.g.nx, ix, S.bx);
  in = wf_axis(0.5 * (y0 + y1), A.g.y0, A.g.hy, A.g.ny, iy, S.by) && in;
  S.bt[0] = 1.0; S.bt[1] = S.bt[2] = S.bt[3] = 0.0;
  if (A.kt > 1) in = wf_axis(tm, A.g.t0, A.g.ht, A.g.nt, it, S.bt) && in;
  S.cell = (it * A.g.ny + iy) * A.g.nx + ix;
  double c0, s0, c1, s1;
  wf_sincos(a0, c0, s0);
  wf_sincos(a1, c1, s1);
  S.mx = (x1 - x0) / dt - 0.5 * (v0 * c0 + v1 * c1);
  S.my = (y1 - y0) / dt - 0.5 * (v0 * s0 + v1 * s1);
  const bool over = !(fabs(S.mx) <= A.p.w_max && fabs(S.my) <= A.p.w_max);
  S.why = !fin ? WF_NONFINITE : !in ? WF_OUTSIDE : over ? WF_OVER : WF_OK;
}

__device__ __forceinline__ double wf_sel4(const double (&b)[4], int k) { return k == 0 ? b[0] : k == 1 ? b[1] : k == 2 ? b[2] : b[3]; }

// The integer rint(x32), x32 = x 2^32 with |x| <= 1, as a double: sums of fewer than 2^20 of them are exact in fp64 (below 2^53)
__device__ __forceinline__ double wf_fix(double x32) { return rint(x32); }
constexpr unsigned WF_WINDOW = 1u << 20;      // samples a wavefront sums in fp64 before it hands the (exact) sums over

// lane s's value of v, s wave-uniform
__device__ __forceinline__ double wf_bcast(double v, int s) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, s), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), s);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ int wf_rows(const FitArgs &A, int f) {
  return A.rows ? min(max(A.rows[f], 0), A.p.n_rows) : A.p.n_rows;
}

// KT = 4: unsteady, NA = 64 sums a lane; KT = 1: steady, NA = 4.
template <int KT>
__global__ void __launch_bounds__(WF_WG, 2)
wf_accum_kernel(FitArgs A) {
#pragma clang fp contract(off)
  constexpr int NA = KT == 4 ? 64 : 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // a workgroup owns a contiguous range of (quad of drones, chunk) pairs, its wavefront w the drone 4 quad + w: the four walk the
  // same rows at about the same time, so the 32 bytes they use of every 128-byte line are fetched once
  const long long u0 = A.n_units * blockIdx.x / gridDim.x, u1 = A.n_units * (blockIdx.x + 1) / gridDim.x;
  const int ny = A.g.ny, nx = A.g.nx, ncp = A.ncp;
  // the lane's column j (its own weight) and, steady, its row group
  const int jb = lane & 3, ja = (lane >> 2) & 3, jc = KT == 4 ? lane >> 4 : 0, grp = lane >> 4;
  double acc[NA], rx = 0.0, ry = 0.0;
  unsigned n_acc = 0;
#pragma unroll
  for (int e = 0; e < NA; ++e) acc[e] = 0.0;
  unsigned cnt_ok = 0, cnt_nf = 0, cnt_out = 0, cnt_over = 0;     // (wave-uniform)
  int cur = -1;

  auto flush = [&]() {
    if (n_acc == 0) return;
    if (KT == 4) {
#pragma unroll
      for (int e = 0; e < 64; ++e) {
        const int c = e >> 4, a = (e >> 2) & 3, b = e & 3;
        const int p = cur + (c * ny + a) * nx + b;
        const int st = ((jc - c + 3) * 7 + (ja - a + 3)) * 7 + (jb - b + 3);
        atomicAdd(A.Hq + (size_t)p * 343 + st, (unsigned long long)(long long)acc[e]);
        acc[e] = 0.0;
      }
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int p = cur + grp * nx + b;
        const int st = (ja - grp + 3) * 7 + (jb - b + 3);
        atomicAdd(A.Hq + (size_t)p * 49 + st, (unsigned long long)(long long)acc[b]);
        acc[b] = 0.0;
      }
    }
    if (KT == 4 || lane < 16) {
      const int p = cur + (jc * ny + ja) * nx + jb;
      atomicAdd(A.bq + p, (unsigned long long)(long long)rx);
      atomicAdd(A.bq + ncp + p, (unsigned long long)(long long)ry);
    }
    rx = ry = 0.0; n_acc = 0;
  };

  for (long long u = u0; u < u1; ++u) {
    const int d = (int)(u / A.n_chunk) * WF_WPB + wave, k = (int)(u % A.n_chunk);
    if (d >= A.N) break;                                      // (uniform: the last quad may be short)
    const int f = d / A.p.n_ac, rows_f = wf_rows(A, f);
    const int i = k * WF_CHUNK + lane;
    if (k * WF_CHUNK + 1 >= rows_f) continue;                 // (uniform: the unit holds no sample)
    WfSample S;
    S.why = -1; S.cell = 0; S.mx = S.my = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) S.bx[q] = S.by[q] = S.bt[q] = 0.0;
    if (i + 1 < rows_f) wf_sample(A, d, f, i, S);
    unsigned long long ok = __ballot(S.why == WF_OK);
    cnt_ok += __popcll(ok);
    cnt_nf += __popcll(__ballot(S.why == WF_NONFINITE));
    cnt_out += __popcll(__ballot(S.why == WF_OUTSIDE));
    cnt_over += __popcll(__ballot(S.why == WF_OVER));
    // the lane's own weight and scaled measurements of ITS sample would be of no use: every lane needs those of sample s
    while (ok) {
      const int s = __builtin_amdgcn_readfirstlane(__ffsll((long long)ok) - 1);      // (wave-uniform: the broadcasts are lane reads)
      ok &= ok - 1;
      const int cell = __builtin_amdgcn_readlane(S.cell, s);
      if (cell != cur || n_acc == WF_WINDOW) { flush(); cur = cell; }
      double bx[4], by[4], bt[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { bx[q] = wf_bcast(S.bx[q], s); by[q] = wf_bcast(S.by[q], s); }
      if (KT == 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) bt[q] = wf_bcast(S.bt[q], s);
      }
      const double mx = wf_bcast(S.mx, s) * A.inv_wp, my = wf_bcast(S.my, s) * A.inv_wp;
      const double wyx = wf_sel4(by, ja) * wf_sel4(bx, jb);
      const double wo = (KT == 4 ? wf_sel4(bt, jc) * wyx : wyx) * WF_SCALE;      // the lane's own weight, times 2^32 (exact)
      if (KT == 4) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double w2 = by[a] * bx[b];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c * 16 + a * 4 + b] += wf_fix((bt[c] * w2) * wo);
          }
      } else {
        const double bg = wf_sel4(by, grp);
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] += wf_fix((bg * bx[b]) * wo);
      }
      rx += wf_fix(wo * mx);
      ry += wf_fix(wo * my);
      ++n_acc;
    }
  }
  flush();
  if (lane == 0) {
    if (cnt_ok) atomicAdd(A.cnt + 0, (unsigned long long)cnt_ok);
    if (cnt_nf) atomicAdd(A.cnt + 1, (unsigned long long)cnt_nf);
    if (cnt_out) atomicAdd(A.cnt + 2, (unsigned long long)cnt_out);
    if (cnt_over) atomicAdd(A.cnt + 3, (unsigned long long)cnt_over);
  }
}

// D^T D of the second differences along an axis of n points (interior differences k = 1 .. n - 2): the entry (a, a + o)
__device__ __forceinline__ double wf_pen(int a, int n, int o) {
  const int q = a + o;
  if (q < 0 || q >= n) return 0.0;
  int sum = 0;
  for (int k = a - 1; k <= a + 1; ++k) {
    if (k < 1 || k > n - 2 || q < k - 1 || q > k + 1) continue;
    sum += (a == k ? -2 : 1) * (q == k ? -2 : 1);
  }
  return (double)sum;
}

__device__ __forceinline__ void wf_point(const FitArgs &A, int p, int &it, int &iy, int &ix) {
  ix = p % A.g.nx; iy = (p / A.g.nx) % A.g.ny; it = p / (A.g.nx * A.g.ny);
}
__device__ __forceinline__ void wf_offset(const FitArgs &A, int st, int &dt, int &dy, int &dx) {
  dx = st % 7 - 3; dy = (st / 7) % 7 - 3; dt = A.kt == 4 ? st / 49 - 3 : 0;
}
__device__ __forceinline__ double wf_prior(const FitArgs &A, int comp, int p) {
  if (!A.g.cp) return 0.0;
  const int plane = A.g.ny * A.g.nx;
  return A.g.cp[(size_t)((p / plane) * 2 + comp) * plane + p % plane];
}

__global__ void __launch_bounds__(256)
wf_convert_kernel(FitArgs A) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n_h = (long long)A.ncp * A.nst;
  const double inv = 1.0 / WF_SCALE;
  if (e < n_h) {
    const int p = (int)(e / A.nst), st = (int)(e % A.nst);
    const double h = (double)(long long)A.Hq[e] * inv;
    int it, iy, ix, dt, dy, dx;
    wf_point(A, p, it, iy, ix);
    wf_offset(A, st, dt, dy, dx);
    double pen = 0.0;
    if (dt == 0 && dy == 0) pen += A.p.lam_x * wf_pen(ix, A.g.nx, dx);
    if (dt == 0 && dx == 0) pen += A.p.lam_y * wf_pen(iy, A.g.ny, dy);
    if (A.kt == 4 && dy == 0 && dx == 0) pen += A.p.lam_t * wf_pen(it, A.g.nt, dt);
    const bool centre = dt == 0 && dy == 0 && dx == 0;
    const int qt = it + dt, qy = iy + dy, qx = ix + dx;
    A.idx[e] = (qt < 0 || qt >= A.g.nt || qy < 0 || qy >= A.g.ny || qx < 0 || qx >= A.g.nx) ? -1 : (qt * A.g.ny + qy) * A.g.nx + qx;
    A.M[e] = h + pen + (centre ? A.p.mu : 0.0);
    if (A.out.H_out) A.out.H_out[e] = h;
    if (centre && A.out.support) A.out.support[p] = h;
  } else if (e < n_h + 2 * A.ncp) {
    const int k = (int)(e - n_h), comp = k / A.ncp, p = k % A.ncp;
    const double b = (double)(long long)A.bq[k] * inv * A.wp;
    A.rhs[k] = b + A.p.mu * wf_prior(A, comp, p);
    if (A.out.b_out) A.out.b_out[k] = b;
  }
}

// sums of v[0 .. 3] over the workgroup in a fixed order: a butterfly inside each wavefront, then the wavefronts in ascending order
__device__ __forceinline__ void wf_reduce4(double (*sh)[WF_CG_WG / 64], double (&v)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    if (lane == 0) sh[k][wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < WF_CG_WG / 64; ++w) t += sh[k][w];
    v[k] = t;
  }
  __syncthreads();
}

// y = M x for both components.  x is staged in LDS (the gather then costs no trip to L2); a wavefront takes four rows at a time,
// lanes along the stencil, so that the loads of four rows are in flight together; a butterfly (fixed order) per row.
template <int NP>                    // stencil entries a lane holds: ceil(nst / 64)
__device__ __forceinline__ void wf_matvec(const FitArgs &A, const double *x, double *y, double *xs) {
  constexpr int WAVES = WF_CG_WG / 64, ROWS = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = A.ncp, nst = A.nst;
  for (int e = threadIdx.x; e < 2 * n; e += WF_CG_WG) xs[e] = x[e];
  __syncthreads();
  for (int p0 = wave * ROWS; p0 < n; p0 += WAVES * ROWS) {
    double m[ROWS][NP];
    int q[ROWS][NP];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const int p = p0 + r, st = lane + 64 * k;
        const bool on = p < n && st < nst;
        const size_t e = (size_t)(on ? p : 0) * nst + (on ? st : 0);
        q[r][k] = on ? A.idx[e] : -1;
        m[r][k] = on ? A.M[e] : 0.0;
      }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const int qq = q[r][k] < 0 ? 0 : q[r][k];
        const double mm = q[r][k] < 0 ? 0.0 : m[r][k];
        s0 = fma(mm, xs[qq], s0); s1 = fma(mm, xs[n + qq], s1);
      }
      for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
      if (lane == 0 && p0 + r < n) { y[p0 + r] = s0; y[n + p0 + r] = s1; }
    }
  }
  __syncthreads();
}

template <int NP>
__global__ void __launch_bounds__(WF_CG_WG)
wf_cg_kernel(FitArgs A) {
  __shared__ double xs[2 * D2D_WINDFIT_MAX_CP];              // 64 KiB: the iterate inside wf_matvec, which rewrites it on entry ...
  double (*sh)[WF_CG_WG / 64] = reinterpret_cast<double (*)[WF_CG_WG / 64]>(xs);   // ... and between two of them the reductions' 32 doubles
  const int tid = threadIdx.x, n = A.ncp;
  double *x = A.vec, *r = x + 2 * n, *pv = r + 2 * n, *Ap = pv + 2 * n, *dinv = Ap + 2 * n;
  const int centre = A.nst / 2;
  for (int p = tid; p < n; p += WF_CG_WG) {
    dinv[p] = 1.0 / A.M[(size_t)p * A.nst + centre];
    x[p] = wf_prior(A, 0, p); x[n + p] = wf_prior(A, 1, p);
  }
  __syncthreads();
  wf_matvec<NP>(A, x, Ap, xs);
  double bb0 = 0.0, bb1 = 0.0, rr0 = 0.0, rr1 = 0.0, rz0 = 0.0, rz1 = 0.0;
  for (int p = tid; p < n; p += WF_CG_WG) {
    const double b0 = A.rhs[p], b1 = A.rhs[n + p], q0 = b0 - Ap[p], q1 = b1 - Ap[n + p];
    r[p] = q0; r[n + p] = q1;
    pv[p] = dinv[p] * q0; pv[n + p] = dinv[p] * q1;
    bb0 = fma(b0, b0, bb0); bb1 = fma(b1, b1, bb1);
    rr0 = fma(q0, q0, rr0); rr1 = fma(q1, q1, rr1);
    rz0 = fma(q0, pv[p], rz0); rz1 = fma(q1, pv[n + p], rz1);
  }
  {
    double v[4] = {bb0, bb1, rr0, rr1}, z[4] = {rz0, rz1, 0.0, 0.0};
    wf_reduce4(sh, v);
    wf_reduce4(sh, z);
    bb0 = v[0]; bb1 = v[1]; rr0 = v[2]; rr1 = v[3]; rz0 = z[0]; rz1 = z[1];
  }
  const double tol2 = A.p.cg_tol * A.p.cg_tol;
  bool done0 = rr0 <= tol2 * bb0, done1 = rr1 <= tol2 * bb1;
  int iters = 0;
  while (iters < A.p.cg_max && !(done0 && done1)) {
    wf_matvec<NP>(A, pv, Ap, xs);
    double pa0 = 0.0, pa1 = 0.0;
    for (int p = tid; p < n; p += WF_CG_WG) { pa0 = fma(pv[p], Ap[p], pa0); pa1 = fma(pv[n + p], Ap[n + p], pa1); }
    {
      double v[4] = {pa0, pa1, 0.0, 0.0};
      wf_reduce4(sh, v);
      pa0 = v[0]; pa1 = v[1];
    }
    const double al0 = done0 || !(pa0 > 0.0) ? 0.0 : rz0 / pa0, al1 = done1 || !(pa1 > 0.0) ? 0.0 : rz1 / pa1;
    double nr0 = 0.0, nr1 = 0.0, nz0 = 0.0, nz1 = 0.0;
    for (int p = tid; p < n; p += WF_CG_WG) {
      x[p] = fma(al0, pv[p], x[p]); x[n + p] = fma(al1, pv[n + p], x[n + p]);
      const double q0 = fma(-al0, Ap[p], r[p]), q1 = fma(-al1, Ap[n + p], r[n + p]);
      r[p] = q0; r[n + p] = q1;
      nr0 = fma(q0, q0, nr0); nr1 = fma(q1, q1, nr1);
      nz0 = fma(q0 * dinv[p], q0, nz0); nz1 = fma(q1 * dinv[p], q1, nz1);
    }
    {
      double v[4] = {nr0, nr1, nz0, nz1};
      wf_reduce4(sh, v);
      nr0 = v[0]; nr1 = v[1]; nz0 = v[2]; nz1 = v[3];
    }
    const double be0 = done0 || !(rz0 > 0.0) ? 0.0 : nz0 / rz0, be1 = done1 || !(rz1 > 0.0) ? 0.0 : nz1 / rz1;
    for (int p = tid; p < n; p += WF_CG_WG) {
      pv[p] = fma(be0, pv[p], dinv[p] * r[p]); pv[n + p] = fma(be1, pv[n + p], dinv[p] * r[n + p]);
    }
    __syncthreads();
    if (!done0) { rr0 = nr0; rz0 = nz0; }
    if (!done1) { rr1 = nr1; rz1 = nz1; }
    done0 = done0 || rr0 <= tol2 * bb0 || !(pa0 > 0.0);
    done1 = done1 || rr1 <= tol2 * bb1 || !(pa1 > 0.0);
    ++iters;
  }
  const int plane = A.g.ny * A.g.nx;
  for (int p = tid; p < n; p += WF_CG_WG) {
    const size_t o = (size_t)(p / plane) * 2 * plane + p % plane;
    A.cp_out[o] = x[p]; A.cp_out[o + plane] = x[n + p];
  }
  if (tid == 0 && A.out.stats) {
    for (int k = 0; k < 4; ++k) A.out.stats[k] = (double)A.cnt[k];
    const double e0 = bb0 > 0.0 ? sqrt(rr0 / bb0) : 0.0, e1 = bb1 > 0.0 ? sqrt(rr1 / bb1) : 0.0;
    A.out.stats[6] = (double)iters;
    A.out.stats[7] = fmax(e0, e1);
  }
}

__global__ void __launch_bounds__(WF_WG)
wf_resid_kernel(FitArgs A) {
  __shared__ double sh[2][WF_WPB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long u0 = A.n_units * blockIdx.x / WF_RES_BLOCKS, u1 = A.n_units * (blockIdx.x + 1) / WF_RES_BLOCKS;
  const int plane = A.g.ny * A.g.nx, nx = A.g.nx;
  double ax = 0.0, ay = 0.0;
  for (long long u = u0; u < u1; ++u) {
    const int d = (int)(u / A.n_chunk) * WF_WPB + wave, k = (int)(u % A.n_chunk);
    if (d >= A.N) break;
    const int f = d / A.p.n_ac, rows_f = wf_rows(A, f);
    const int i = k * WF_CHUNK + lane;
    if (i + 1 >= rows_f) continue;
    WfSample S;
    wf_sample(A, d, f, i, S);
    if (S.why != WF_OK) continue;
    const int ct = S.cell / plane, cr = S.cell % plane;
    double fx = 0.0, fy = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= A.kt) break;
      const double *base = A.cp_out + (size_t)(ct + c) * 2 * plane + cr;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double w = S.bt[c] * (S.by[a] * S.bx[b]);
          fx = fma(w, base[a * nx + b], fx); fy = fma(w, base[plane + a * nx + b], fy);
        }
    }
    const double ex = fx - S.mx, ey = fy - S.my;
    ax = fma(ex, ex, ax); ay = fma(ey, ey, ay);
  }
  for (int o = 32; o > 0; o >>= 1) { ax += __shfl_xor(ax, o); ay += __shfl_xor(ay, o); }
  if (lane == 0) { sh[0][wave] = ax; sh[1][wave] = ay; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sx = 0.0, sy = 0.0;
    for (int w = 0; w < WF_WPB; ++w) { sx += sh[0][w]; sy += sh[1][w]; }
    A.part[2 * blockIdx.x] = sx; A.part[2 * blockIdx.x + 1] = sy;
  }
}

__global__ void wf_fold_kernel(FitArgs A) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sx = 0.0, sy = 0.0;
  for (int b = 0; b < WF_RES_BLOCKS; ++b) { sx += A.part[2 * b]; sy += A.part[2 * b + 1]; }
  A.out.stats[4] = sx; A.out.stats[5] = sy;
}

size_t wf_align(size_t n) { return (n + 15) / 16 * 16; }
size_t wf_q_bytes(const FitArgs &A) { return wf_align(((size_t)A.ncp * A.nst + 2 * (size_t)A.ncp + 4) * sizeof(unsigned long long)); }
size_t wf_m_bytes(const FitArgs &A) { return wf_align(((size_t)A.ncp * A.nst + 2 * (size_t)A.ncp) * sizeof(double)); }
size_t wf_vec_bytes(const FitArgs &A) { return wf_align((size_t)A.ncp * 9 * sizeof(double)); }
size_t wf_part_bytes() { return wf_align((size_t)WF_RES_BLOCKS * 2 * sizeof(double)); }
size_t wf_idx_bytes(const FitArgs &A) { return wf_align((size_t)A.ncp * A.nst * sizeof(int32_t)); }

// what makes the arguments D2D_EINVAL (include/d2d.h), and the launch geometry they give
int wf_plan(const d2d_windfit_params *p, const d2d_wind_field *g, const char *who, FitArgs &A) {
  D2D_REQUIRE(p && g, "%s: null parameters or grid", who);
  D2D_REQUIRE(g->nx >= 4 && g->ny >= 4 && (g->nt == 1 || g->nt >= 4), "%s: grid nt=%d, ny=%d, nx=%d (nx, ny >= 4; nt = 1 or >= 4)", who,
              g->nt, g->ny, g->nx);
  D2D_REQUIRE(g->hx > 0 && g->hy > 0 && (g->nt == 1 || g->ht > 0), "%s: grid knot spacings must be > 0", who);
  D2D_REQUIRE(std::isfinite(g->x0) && std::isfinite(g->hx) && std::isfinite(g->y0) && std::isfinite(g->hy)
              && (g->nt == 1 || (std::isfinite(g->t0) && std::isfinite(g->ht))), "%s: grid knots must be finite", who);
  const long long ncp = (long long)g->nt * g->ny * g->nx;
  D2D_REQUIRE(ncp <= D2D_WINDFIT_MAX_CP, "%s: %lld control points, at most %d", who, ncp, D2D_WINDFIT_MAX_CP);
  D2D_REQUIRE(p->n_form >= 1 && p->n_ac >= 1 && p->n_ac <= 64 && p->n_rows >= 2,
              "%s: n_form >= 1, n_ac in 1 .. 64 and n_rows >= 2 required (n_form=%d n_ac=%d n_rows=%d)", who, p->n_form, p->n_ac, p->n_rows);
  D2D_REQUIRE(p->dt_row > 0 && std::isfinite(p->dt_row) && p->w_max > 0 && std::isfinite(p->w_max) && p->mu > 0 && std::isfinite(p->mu),
              "%s: dt_row, w_max and mu must be finite and > 0 (%g, %g, %g)", who, p->dt_row, p->w_max, p->mu);
  D2D_REQUIRE(p->lam_x >= 0 && std::isfinite(p->lam_x) && p->lam_y >= 0 && std::isfinite(p->lam_y) && p->lam_t >= 0 && std::isfinite(p->lam_t),
              "%s: lam_x, lam_y, lam_t must be finite and >= 0", who);
  D2D_REQUIRE(p->cg_tol > 0 && p->cg_tol < 1 && p->cg_max >= 1, "%s: cg_tol in (0, 1) and cg_max >= 1 required (%g, %d)", who, p->cg_tol, p->cg_max);
  D2D_REQUIRE(p->waves >= 0, "%s: waves = %d (0: the library's choice)", who, p->waves);
  const long long N = (long long)p->n_form * p->n_ac;
  D2D_REQUIRE((long long)(p->n_rows - 1) * N < (1LL << 31), "%s: (n_rows - 1) N = %lld samples, fewer than 2^31 required (the 64-bit sums)", who,
              (long long)(p->n_rows - 1) * N);
  int e = 0;
  const double fr = std::frexp(p->w_max, &e);                // w_max = fr 2^e, fr in [0.5, 1)
  A.wp = std::ldexp(1.0, fr == 0.5 ? e - 1 : e);
  D2D_REQUIRE(std::isfinite(A.wp) && A.wp >= 1e-300, "%s: w_max = %g out of range", who, p->w_max);
  A.inv_wp = 1.0 / A.wp;
  A.p = *p; A.g = *g;
  A.N = (int)N; A.kt = g->nt == 1 ? 1 : 4; A.nst = g->nt == 1 ? 49 : 343; A.ncp = (int)ncp;
  A.n_chunk = (p->n_rows - 1 + WF_CHUNK - 1) / WF_CHUNK;
  A.n_units = (N + WF_WPB - 1) / WF_WPB * A.n_chunk;         // (quad of drones, chunk) pairs: one per workgroup and step
  const long long want = ((p->waves > 0 ? p->waves : WF_WAVES) + WF_WPB - 1) / WF_WPB;
  A.n_waves = (int)std::max(1LL, std::min(want, A.n_units)) * WF_WPB;
  return D2D_OK;
}

}  // namespace

extern "C" {

int64_t d2d_wind_fit_workspace(const d2d_windfit_params *p, const d2d_wind_field *grid) {
  FitArgs A{};
  if (wf_plan(p, grid, "d2d_wind_fit_workspace", A)) return D2D_EINVAL;
  return (int64_t)(wf_q_bytes(A) + wf_m_bytes(A) + wf_vec_bytes(A) + wf_part_bytes() + wf_idx_bytes(A));
}

int d2d_wind_fit(d2d_ctx *ctx, const d2d_windfit_params *p, const double *X_hist, const int32_t *rows, const double *t_start,
                 const d2d_wind_field *grid, double *cp_out, void *work, const d2d_windfit_out *out) {
  D2D_REQUIRE(ctx && p && X_hist && grid && cp_out && work, "d2d_wind_fit: null argument (ctx, p, X_hist, grid, cp_out or work)");
  FitArgs A{};
  if (int rc = wf_plan(p, grid, "d2d_wind_fit", A)) return rc;
  A.X = X_hist; A.rows = rows; A.t_start = t_start; A.cp_out = cp_out;
  if (out) A.out = *out;
  char *w = static_cast<char *>(work);
  A.Hq = reinterpret_cast<unsigned long long *>(w);
  A.bq = A.Hq + (size_t)A.ncp * A.nst;
  A.cnt = A.bq + 2 * (size_t)A.ncp;
  w += wf_q_bytes(A);
  A.M = reinterpret_cast<double *>(w);
  A.rhs = A.M + (size_t)A.ncp * A.nst;
  w += wf_m_bytes(A);
  A.vec = reinterpret_cast<double *>(w);
  w += wf_vec_bytes(A);
  A.part = reinterpret_cast<double *>(w);
  w += wf_part_bytes();
  A.idx = reinterpret_cast<int32_t *>(w);
  D2D_CHECK_HIP(hipMemsetAsync(A.Hq, 0, wf_q_bytes(A), ctx->stream));
  const unsigned blocks = (unsigned)(A.n_waves / WF_WPB);
  if (A.kt == 4) hipLaunchKernelGGL(wf_accum_kernel<4>, dim3(blocks), dim3(WF_WG), 0, ctx->stream, A);
  else hipLaunchKernelGGL(wf_accum_kernel<1>, dim3(blocks), dim3(WF_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  const long long n_conv = (long long)A.ncp * A.nst + 2 * A.ncp;
  hipLaunchKernelGGL(wf_convert_kernel, dim3((unsigned)((n_conv + 255) / 256)), dim3(256), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  if (A.kt == 4) hipLaunchKernelGGL(wf_cg_kernel<6>, dim3(1), dim3(WF_CG_WG), 0, ctx->stream, A);
  else hipLaunchKernelGGL(wf_cg_kernel<1>, dim3(1), dim3(WF_CG_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  if (A.out.stats) {
    hipLaunchKernelGGL(wf_resid_kernel, dim3(WF_RES_BLOCKS), dim3(WF_WG), 0, ctx->stream, A);
    D2D_LAUNCH_CHECK();
    hipLaunchKernelGGL(wf_fold_kernel, dim3(1), dim3(64), 0, ctx->stream, A);
    D2D_LAUNCH_CHECK();
  }
  return D2D_OK;
}

}  // extern "C"
