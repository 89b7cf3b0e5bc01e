// Device evaluation of wind fields (include/d2d.h d2d_wind_field): shared by the plant loops (sim_device.h) and the collocation
// planner (nlp_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/d2d.h"

// ---- wind fields (include/d2d.h d2d_wind_field): uniform tensor-product cubic B-splines ----------------------------------------
// One axis: the segment i of the coordinate u (clamped to the spline's box) and the four B-spline weights of c[i .. i+3].  A NaN
// coordinate is clamped to the box as well (fmax(NaN, 0) = 0): every index stays inside the control-point table.
__device__ __forceinline__ int wind_axis(double u, double u0, double h, int n, double (&b)[4]) {
  double s = (u - u0) / h;
  s = fmin(fmax(s, 0.0), (double)(n - 3));
  const double fl = fmin(floor(s), (double)(n - 4));
  const double r = s - fl, q = 1.0 - r, r2 = r * r, r3 = r2 * r;
  b[0] = q * q * q * (1.0 / 6.0);
  b[1] = (3.0 * r3 - 6.0 * r2 + 4.0) * (1.0 / 6.0);
  b[2] = (-3.0 * r3 + 3.0 * r2 + 3.0 * r + 1.0) * (1.0 / 6.0);
  b[3] = r3 * (1.0 / 6.0);
  return (int)fl;
}

struct WindVec { double x, y; };   // (returned in registers)

// The field at (t, x, y): 4 x 4 (steady) or 4 x 4 x 4 (unsteady; the time slices in a rolled loop) weighted control points per
// component.  Inlined: as an out-of-line call from the divergent mesh branches of plant_step, the general formation kernel's results
// changed from run to run once a wavefront mixed the two branches; inlined, they match the CPU statement to rounding.
__device__ __forceinline__ WindVec wind_eval(const double *__restrict__ cp, int nt, int ny, int nx, double t0, double ht, double x0,
                                          double hx, double y0, double hy, double t, double x, double y) {
  double bx[4], by[4];
  const int ix = wind_axis(x, x0, hx, nx, bx), iy = wind_axis(y, y0, hy, ny, by);
  const long plane = (long)ny * nx;
  WindVec o = {0.0, 0.0};
  double bt[4] = {1.0, 0.0, 0.0, 0.0};
  int it = 0, kt = 1;
  if (nt > 1) { it = wind_axis(t, t0, ht, nt, bt); kt = 4; }
  for (int c = 0; c < kt; ++c) {
    const double *r0 = cp + (long)(it + c) * 2 * plane + (long)iy * nx + ix;
    double ax = 0.0, ay = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const double *rx = r0 + (long)a * nx, *ry = rx + plane;
      const double sx = bx[0] * rx[0] + bx[1] * rx[1] + bx[2] * rx[2] + bx[3] * rx[3];
      const double sy = bx[0] * ry[0] + bx[1] * ry[1] + bx[2] * ry[2] + bx[3] * ry[3];
      ax += by[a] * sx;
      ay += by[a] * sy;
    }
    o.x += bt[c] * ax;
    o.y += bt[c] * ay;
  }
  return o;
}

__device__ __forceinline__ WindVec wind_at(const d2d_wind_field &f, double t, double x, double y) {
  return wind_eval(f.cp, f.nt, f.ny, f.nx, f.t0, f.ht, f.x0, f.hx, f.y0, f.hy, t, x, y);
}

// One axis with derivatives: wind_axis plus the weights B_k'(r) / h and B_k''(r) / h^2.  Along a clamped coordinate (a query outside
// the box, or NaN) both are zero: they are the derivatives of the clamped field (d2d/wind.py _weights_d).
__device__ __forceinline__ int wind_axis2(double u, double u0, double h, int n, double (&b)[4], double (&d1)[4], double (&d2)[4]) {
  const double sr = (u - u0) / h;
  const double s = fmin(fmax(sr, 0.0), (double)(n - 3));
  const double fl = fmin(floor(s), (double)(n - 4));
  const double r = s - fl, q = 1.0 - r, r2 = r * r, r3 = r2 * r;
  b[0] = q * q * q * (1.0 / 6.0);
  b[1] = (3.0 * r3 - 6.0 * r2 + 4.0) * (1.0 / 6.0);
  b[2] = (-3.0 * r3 + 3.0 * r2 + 3.0 * r + 1.0) * (1.0 / 6.0);
  b[3] = r3 * (1.0 / 6.0);
  const bool inside = sr >= 0.0 && sr <= (double)(n - 3);
  const double i1 = inside ? 1.0 / h : 0.0, i2 = inside ? 1.0 / (h * h) : 0.0;
  d1[0] = -0.5 * q * q * i1; d1[1] = (1.5 * r2 - 2.0 * r) * i1; d1[2] = (-1.5 * r2 + r + 0.5) * i1; d1[3] = 0.5 * r2 * i1;
  d2[0] = q * i2; d2[1] = (3.0 * r - 2.0) * i2; d2[2] = (1.0 - 3.0 * r) * i2; d2[3] = r * i2;
  return (int)fl;
}

// Value, spatial Jacobian and spatial second derivatives of both components at (t, x, y), one pass over the 16 (steady) or 64
// (unsteady) control-point pairs: w, d/dx, d/dy, d2/dx2, d2/dxdy, d2/dy2.  The device twin of SplineWindField.derivatives (d2d/wind.py),
// sum for sum; the value is wind_eval's.  Inlined, like wind_eval.
struct WindJet {
  double w[2], dx[2], dy[2], xx[2], xy[2], yy[2];
};

__device__ __forceinline__ WindJet wind_eval2(const d2d_wind_field &f, double t, double x, double y) {
  WindJet o = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
  double bx[4], by[4], ex[4], ey[4], fx[4], fy[4];
  const int nx = f.nx, ny = f.ny;
  const int ix = wind_axis2(x, f.x0, f.hx, nx, bx, ex, fx), iy = wind_axis2(y, f.y0, f.hy, ny, by, ey, fy);
  const long plane = (long)ny * nx;
  double bt[4] = {1.0, 0.0, 0.0, 0.0};
  int it = 0, kt = 1;
  if (f.nt > 1) { it = wind_axis(t, f.t0, f.ht, f.nt, bt); kt = 4; }
  for (int c = 0; c < kt; ++c) {
    const double *r0 = f.cp + (long)(it + c) * 2 * plane + (long)iy * nx + ix;
    double a[6][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double *r = r0 + (long)j * nx + (long)k * plane;
        const double c0 = r[0], c1 = r[1], c2 = r[2], c3 = r[3];
        const double s0 = bx[0] * c0 + bx[1] * c1 + bx[2] * c2 + bx[3] * c3;
        const double s1 = ex[0] * c0 + ex[1] * c1 + ex[2] * c2 + ex[3] * c3;
        const double s2 = fx[0] * c0 + fx[1] * c1 + fx[2] * c2 + fx[3] * c3;
        a[0][k] += by[j] * s0; a[1][k] += by[j] * s1; a[2][k] += ey[j] * s0;
        a[3][k] += by[j] * s2; a[4][k] += ey[j] * s1; a[5][k] += fy[j] * s0;
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      o.w[k] += bt[c] * a[0][k]; o.dx[k] += bt[c] * a[1][k]; o.dy[k] += bt[c] * a[2][k];
      o.xx[k] += bt[c] * a[3][k]; o.xy[k] += bt[c] * a[4][k]; o.yy[k] += bt[c] * a[5][k];
    }
  }
  return o;
}
