// Gust dispersion of LQR-tracked plans (include/d2d.h d2d_track_dispersion): the covariance of the tracking error of
// d2d_sim_track_run_gust, propagated row by row without sampling.  One drone per lane, as in track_run_body; the gain of a row is
// compute_gain's (sim_device.h), the plant's Jacobian is the true one, the step is an exact zero-order hold.
// tests/dispersion_ref.py is the CPU statement.
#include <cmath>

#include "common.h"
#include "sim_device.h"

namespace {

// The zero-order-hold integrals of the two actuator lags over one step h -- launch constants, computed by the host in long double.
// With z = h / tau and phi_k the functions phi_1(x) = (e^x - 1) / x, phi_2(x) = (e^x - 1 - x) / x^2, phi_3(x) = (e^x - 1 - x - x^2/2) / x^3:
//   e  = exp(-z)                                 the lag's own decay
//   m0 = 1 - e                     = z phi_1(-z)          (the hold's share of the lag itself)
//   i1 = int_0^h exp(-t/tau) dt    = h phi_1(-z)
//   m1 = h - i1                    = h z phi_2(-z)        (the hold's share of the first integral)
//   j1 = int_0^h i1(t) dt          = h^2 phi_2(-z)
//   k1 = h^2 / 2 - j1              = h^2 z phi_3(-z)      (the hold's share of the second integral)
// Written with the phi functions none of them is a difference of nearly equal numbers, whatever z (tau_phi = 0.01 s: z = 5 .. 10;
// tau_v = 1 s: z = 0.05).
struct LagInts {
  double e, m0, i1, m1, j1, k1;
};
struct DispConsts {
  LagInts phi, v;
  double h;
};

LagInts lag_ints(double h, double tau) {
  const long double z = (long double)h / (long double)tau, x = -z;
  long double p1, p2, p3;
  if (z < 0.5L) {                                  // Taylor series of phi_3, then the stable recurrences phi_k = x phi_{k+1} + 1 / k!
    long double term = 1.0L / 6.0L, sum = 0.0L;    // x^k / (k + 3)!
    for (int k = 0; k < 24; ++k) { sum += term; term *= x / (long double)(k + 4); }
    p3 = sum; p2 = x * p3 + 0.5L; p1 = x * p2 + 1.0L;
  } else {                                         // e^x <= 0.61: the differences below lose at most two bits
    p1 = expm1l(x) / x; p2 = (p1 - 1.0L) / x; p3 = (p2 - 0.5L) / x;
  }
  const long double hl = h;
  LagInts r;
  r.e = (double)(x * p1 + 1.0L);
  r.m0 = (double)(z * p1);
  r.i1 = (double)(hl * p1);
  r.m1 = (double)(hl * z * p2);
  r.j1 = (double)(hl * hl * p2);
  r.k1 = (double)(hl * hl * z * p3);
  return r;
}

// numpy.gradient(f, edge_order=2) / dt at row i of a [T][n] plane, the tracking loop's derivative (gradient_kernel of sim_kernels.hip);
// T = 2 has no second-order edge formula: the one difference f_1 - f_0 on both rows (numpy.gradient's edge_order=1)
__global__ void __launch_bounds__(256) disp_gradient_kernel(int T, int n, double inv_dt, const double *__restrict__ f, double *__restrict__ out) {
  const long d = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (d >= n) return;
  double g;
  if (T == 2) g = f[n + d] - f[d];
  else if (i == 0) g = -1.5 * f[d] + 2.0 * f[n + d] - 0.5 * f[2L * n + d];
  else if (i == T - 1) g = 1.5 * f[(long)(T - 1) * n + d] - 2.0 * f[(long)(T - 2) * n + d] + 0.5 * f[(long)(T - 3) * n + d];
  else g = 0.5 * (f[(long)(i + 1) * n + d] - f[(long)(i - 1) * n + d]);
  out[(long)i * n + d] = g * inv_dt;
}

struct DispArgs {
  d2d_track_params p;
  DispConsts c;
  double a, s2, sigma2;                   // the gust: a, s^2, sigma^2
  const double *x_ref, *y_ref, *xd, *yd, *xdd, *ydd;
  const double *S_in;
  int n_edge, n_keep;
  const double *edges, *discs;
  d2d_dispersion_out o;
};

// packed lower triangle: entry (i, j), i >= j
__host__ __device__ constexpr int tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// Row i of the recursion  S_i = F_i S_{i-1} F_i^T + diag(0_5, s^2, s^2),  F_i = [[Acl, Ed], [0, a I_2]],  Acl = Ad - Bd K_i,
// on the blocks S = [[P, C], [C^T, G]] (P 5x5, C 5x2, G 2x2), Ed = h [I_2; 0]:
//   T = Acl P + Ed C^T,  D = Acl C + Ed G,  P' = T Acl^T + D Ed^T,  C' = a D,  G' = a^2 G + s^2 I
// Only the 28 packed entries are carried: S stays symmetric by construction.
__device__ __forceinline__ void disp_step(double (&S)[28], const double (&Acl)[5][5], double h, double a, double s2) {
  double T[5][5], D[5][2];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double t = (i < 2) ? h * S[tri(5 + i, k)] : 0.0;
#pragma unroll
      for (int m = 0; m < 5; ++m) t = fma(Acl[i][m], S[tri(m, k)], t);
      T[i][k] = t;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      double t = (i < 2) ? h * S[tri(5 + i, 5 + c)] : 0.0;
#pragma unroll
      for (int m = 0; m < 5; ++m) t = fma(Acl[i][m], S[tri(5 + c, m)], t);
      D[i][c] = t;
    }
  }
  double N[28];
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double t = (j < 2) ? h * D[i][j] : 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) t = fma(T[i][k], Acl[j][k], t);
      N[tri(i, j)] = t;
    }
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < 5; ++i) N[tri(5 + c, i)] = a * D[i][c];
  const double a2 = a * a;
  N[tri(5, 5)] = fma(a2, S[tri(5, 5)], s2);
  N[tri(6, 5)] = a2 * S[tri(6, 5)];
  N[tri(6, 6)] = fma(a2, S[tri(6, 6)], s2);
#pragma unroll
  for (int q = 0; q < 28; ++q) S[q] = N[q];
}

__global__ void __launch_bounds__(64) track_dispersion_kernel(DispArgs A) {
  const d2d_track_params &p = A.p;
  const long n = p.n;
  long d = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const bool live = d < n;
  if (!live) d = n - 1;                               // (keeps the wave converged in care_sda_diag's votes, as the tracking loop does)
  double S[28];
#pragma unroll
  for (int q = 0; q < 28; ++q) S[q] = A.S_in ? A.S_in[(long)q * n + d] : 0.0;
  if (!A.S_in) { S[tri(5, 5)] = A.sigma2; S[tri(6, 6)] = A.sigma2; }   // the stationary start of gust_begin
  const d2d_dispersion_out &o = A.o;
  if (live && o.Ppos_hist) { o.Ppos_hist[d] = S[tri(0, 0)]; o.Ppos_hist[n + d] = S[tri(1, 0)]; o.Ppos_hist[2 * n + d] = S[tri(1, 1)]; }
  const double h = A.c.h;
  const LagInts &lp = A.c.phi, &lv = A.c.v;
  const double inf = __builtin_inf();
  double sig_max = -1.0;
  int sig_row = 1;
  for (int i = 1; i < p.n_rows; ++i) {
    const long r = (long)i * n + d;
    const double Y[8] = {A.x_ref[r], A.y_ref[r], A.xd[r], A.yd[r], A.xdd[r], A.ydd[r], 0.0, 0.0};   // Yddd = 0, as flown
    const State5 X0 = {0.0, 0.0, 0.0, 0.0, 0.0};      // the gain does not depend on the state: only o.Xr and o.K are used
    const GainOut g = compute_gain(X0, Y, p);
    // the plant's own Jacobian at Xr (oracle/sim.py cont_dyn), NOT cont_jac's quirk entries: those belong to the controller
    double spsi, cpsi, sphi, cphi;
    sincos(g.Xr.psi, &spsi, &cpsi);
    sincos(g.Xr.phi, &sphi, &cphi);
    const double v = g.Xr.v;
    const double ax = -v * spsi, ay = v * cpsi;                         // d x' / d psi, d y' / d psi
    const double pj = D2D_G / (v * cphi * cphi), qj = -D2D_G * (sphi / cphi) / (v * v);   // d psi' / d phi, d psi' / d v
    // [Ad Bd Ed] = the first five rows of expm(dt [[A B E], [0 0 0]]) in closed form: columns 0 and 1 of A are zero and phi, v are
    // decoupled lags, so psi is one and (x, y) two integrals of exponentials (LagInts)
    double Ad[5][5], Bd[5][2];
#pragma unroll
    for (int a_ = 0; a_ < 5; ++a_) {
#pragma unroll
      for (int b_ = 0; b_ < 5; ++b_) Ad[a_][b_] = (a_ == b_ && a_ < 3) ? 1.0 : 0.0;
      Bd[a_][0] = 0.0; Bd[a_][1] = 0.0;
    }
    Ad[3][3] = lp.e; Bd[3][0] = lp.m0;
    Ad[4][4] = lv.e; Bd[4][1] = lv.m0;
    Ad[2][3] = pj * lp.i1; Ad[2][4] = qj * lv.i1;
    Bd[2][0] = pj * lp.m1; Bd[2][1] = qj * lv.m1;
    const double x3 = pj * lp.j1, x4 = qj * lv.j1, u0 = pj * lp.k1, u1 = qj * lv.k1;   // int_0^h psi per unit of phi_0, v_0, u_phi, u_v
    Ad[0][2] = ax * h; Ad[0][3] = ax * x3; Ad[0][4] = fma(ax, x4, cpsi * lv.i1);
    Ad[1][2] = ay * h; Ad[1][3] = ay * x3; Ad[1][4] = fma(ay, x4, spsi * lv.i1);
    Bd[0][0] = ax * u0; Bd[0][1] = fma(ax, u1, cpsi * lv.m1);
    Bd[1][0] = ay * u0; Bd[1][1] = fma(ay, u1, spsi * lv.m1);
    double Acl[5][5];
#pragma unroll
    for (int a_ = 0; a_ < 5; ++a_)
#pragma unroll
      for (int b_ = 0; b_ < 5; ++b_) Acl[a_][b_] = fma(-Bd[a_][1], g.K[1][b_], fma(-Bd[a_][0], g.K[0][b_], Ad[a_][b_]));
    disp_step(S, Acl, h, A.a, A.s2);
    if (!live) continue;
    const double xx = S[tri(0, 0)], xy = S[tri(1, 0)], yy = S[tri(1, 1)];
    if (o.Ppos_hist) {
      double *P3 = o.Ppos_hist + (long)i * 3 * n;
      P3[d] = xx; P3[n + d] = xy; P3[2 * n + d] = yy;
    }
    {                                                 // sqrt(lambda_max) of the position block
      const double hd = 0.5 * (xx - yy);
      const double sg = sqrt(fmax(fma(0.5, xx + yy, sqrt(fma(hd, hd, xy * xy))), 0.0));
      if (sg > sig_max) { sig_max = sg; sig_row = i; }
    }
    const double px = Y[0], py = Y[1];
    for (int e = 0; e < A.n_edge; ++e) {              // running extremes live in the outputs: no lane-indexed arrays in registers
      const double *ed = A.edges + ((long)d * A.n_edge + e) * 4;
      const double ex = ed[0], ey = ed[1];
      const long q = (long)e * n + d;
      const bool absent = ex == 0.0 && ey == 0.0;
      const double var = fma(ex, fma(ex, xx, ey * xy), ey * fma(ex, xy, ey * yy));
      const double sn = absent ? 0.0 : sqrt(fmax(var, 0.0));
      if (o.fence_sn) o.fence_sn[q] = (i == 1) ? sn : fmax(o.fence_sn[q], sn);
      if (o.fence_k) {
        const double k = (absent || !(sn > 0.0)) ? inf : (ed[2] - fma(ex, px, ey * py)) / sn;
        if (i == 1) { o.fence_k[q] = k; o.fence_row[q] = absent ? -1 : 1; }
        else if (k < o.fence_k[q]) { o.fence_k[q] = k; o.fence_row[q] = i; }
      }
    }
    if (o.disc_k) {
      for (int m = 0; m < A.n_keep; ++m) {
        const double *dc = A.discs + ((long)d * A.n_keep + m) * 3;
        const long q = (long)m * n + d;
        const bool absent = !(dc[2] > 0.0);
        const double rx = px - dc[0], ry = py - dc[1], dist = sqrt(fma(rx, rx, ry * ry));
        const double ux = rx / dist, uy = ry / dist;
        const double sn = sqrt(fmax(fma(ux, fma(ux, xx, uy * xy), uy * fma(ux, xy, uy * yy)), 0.0));
        const double k = (absent || !(sn > 0.0)) ? inf : (dist - dc[2]) / sn;
        if (i == 1) { o.disc_k[q] = k; o.disc_row[q] = absent ? -1 : 1; }
        else if (k < o.disc_k[q]) { o.disc_k[q] = k; o.disc_row[q] = i; }
      }
    }
  }
  if (!live) return;
  if (o.sig_max) o.sig_max[d] = sig_max;
  if (o.sig_row) o.sig_row[d] = sig_row;
  if (o.S_out) {
#pragma unroll
    for (int q = 0; q < 28; ++q) o.S_out[(long)q * n + d] = S[q];
  }
}

}  // namespace

extern "C" {

int d2d_track_dispersion(d2d_ctx *ctx, const d2d_track_params *p, const double *x_ref, const double *y_ref, const d2d_dispersion_in *in,
                         const d2d_fence *fence, const d2d_keep_out *keep, const d2d_dispersion_out *out) {
  const char *who = "d2d_track_dispersion";
  D2D_REQUIRE(ctx && p && x_ref && y_ref, "%s: null argument (ctx, p, x_ref or y_ref)", who);
  D2D_REQUIRE(in && out, "%s: null input or output struct", who);
  D2D_REQUIRE(p->n >= 1 && p->n_rows >= 2, "%s: n >= 1 and n_rows >= 2 required (n=%d n_rows=%d)", who, p->n, p->n_rows);
  D2D_REQUIRE(p->dt > 0 && std::isfinite(p->dt) && p->tau_phi > 0 && p->tau_v > 0, "%s: dt, tau_phi, tau_v must be > 0", who);
  D2D_REQUIRE(p->r_diag[0] > 0 && p->r_diag[1] > 0, "%s: R must be positive", who);
  D2D_REQUIRE(in->a >= 0 && in->a < 1, "%s: gust a=%g not in [0, 1)", who, in->a);
  D2D_REQUIRE(std::isfinite(in->s) && in->s >= 0 && std::isfinite(in->sigma) && in->sigma >= 0, "%s: gust s, sigma must be finite and >= 0", who);
  const int n_edge = fence ? fence->n_edge : 0, n_keep = keep ? keep->n_keep : 0;
  D2D_REQUIRE(n_edge >= 0 && n_edge <= D2D_MAX_FENCE, "%s: n_edge=%d outside 0 .. %d", who, n_edge, D2D_MAX_FENCE);
  D2D_REQUIRE(n_keep >= 0 && n_keep <= D2D_MAX_KEEP, "%s: n_keep=%d outside 0 .. %d", who, n_keep, D2D_MAX_KEEP);
  D2D_REQUIRE(n_edge == 0 || fence->edges, "%s: n_edge=%d with NULL edges", who, n_edge);
  D2D_REQUIRE(n_keep == 0 || keep->discs, "%s: n_keep=%d with NULL discs", who, n_keep);
  D2D_REQUIRE(n_edge > 0 || !(out->fence_sn || out->fence_k || out->fence_row), "%s: a fence output without fence edges", who);
  D2D_REQUIRE(n_keep > 0 || !(out->disc_k || out->disc_row), "%s: a disc output without keep-out discs", who);
  D2D_REQUIRE(!out->fence_k == !out->fence_row, "%s: fence_k and fence_row go together", who);
  D2D_REQUIRE(!out->disc_k == !out->disc_row, "%s: disc_k and disc_row go together", who);
  DispArgs A{};
  A.p = *p;
  A.c.h = p->dt; A.c.phi = lag_ints(p->dt, p->tau_phi); A.c.v = lag_ints(p->dt, p->tau_v);
  A.a = in->a; A.s2 = in->s * in->s; A.sigma2 = in->sigma * in->sigma;
  A.S_in = in->S_in;
  A.n_edge = (out->fence_sn || out->fence_k) ? n_edge : 0;
  A.n_keep = out->disc_k ? n_keep : 0;
  A.edges = n_edge ? fence->edges : nullptr; A.discs = n_keep ? keep->discs : nullptr;
  A.o = *out;
  const size_t plane = (size_t)p->n_rows * p->n;
  double *deriv = nullptr;
  D2D_CHECK_HIP(hipMallocAsync(reinterpret_cast<void **>(&deriv), 4 * plane * sizeof(double), ctx->stream));
  double *xd = deriv, *yd = deriv + plane, *xdd = deriv + 2 * plane, *ydd = deriv + 3 * plane;
  const dim3 g((p->n + 255) / 256, p->n_rows), b(256);
  const double inv_dt = 1.0 / p->dt;
  hipLaunchKernelGGL(disp_gradient_kernel, g, b, 0, ctx->stream, p->n_rows, p->n, inv_dt, x_ref, xd);
  hipLaunchKernelGGL(disp_gradient_kernel, g, b, 0, ctx->stream, p->n_rows, p->n, inv_dt, y_ref, yd);
  hipLaunchKernelGGL(disp_gradient_kernel, g, b, 0, ctx->stream, p->n_rows, p->n, inv_dt, xd, xdd);
  hipLaunchKernelGGL(disp_gradient_kernel, g, b, 0, ctx->stream, p->n_rows, p->n, inv_dt, yd, ydd);
  A.x_ref = x_ref; A.y_ref = y_ref; A.xd = xd; A.yd = yd; A.xdd = xdd; A.ydd = ydd;
  hipLaunchKernelGGL(track_dispersion_kernel, dim3((p->n + 63) / 64), dim3(64), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  D2D_CHECK_HIP(hipFreeAsync(deriv, ctx->stream));
  return D2D_OK;
}

}  // extern "C"
