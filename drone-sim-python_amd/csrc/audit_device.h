// The candidates of a segment of relative motion and the order of their keys: ONE sequence of operations, shared by the in-formation
// audit (audit_kernels.hip) and the fleet audit (fleet_audit.hip), so that the same pair of paths gives the same bits in both.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ bool aud_finite(double v) { return fabs(v) <= 1.79e308; }
__device__ __forceinline__ double aud_inf() { return __builtin_huge_val(); }
__device__ __forceinline__ double aud_nan() { return __builtin_nan(""); }

// key (d2, u, j) < (bd2, bu, bj): the smaller distance, then the earlier time, then the smaller partner
__device__ __forceinline__ bool aud_less(double d2, double u, int j, double bd2, double bu, int bj) {
  return d2 < bd2 || (d2 == bd2 && (u < bu || (u == bu && j < bj)));
}

// The candidates of the relative position p0 at row i (and p1 at row i + 1 when the segment exists) against the best key so far.
// Returns the row's own squared distance.
__device__ __forceinline__ double aud_segment(double p0x, double p0y, double p1x, double p1y, bool seg, int i, int j,
                                              double &bd2, double &bu, int &bj) {
  const double r2 = fma(p0x, p0x, p0y * p0y);
  const double ui = (double)i;
  if (aud_less(r2, ui, j, bd2, bu, bj)) { bd2 = r2; bu = ui; bj = j; }
  if (seg) {
    const double dx = p1x - p0x, dy = p1y - p0y;
    const double num = -fma(p0x, dx, p0y * dy), dd = fma(dx, dx, dy * dy);
    if (num > 0.0 && num < dd) {             // 0 < s* < 1 (dd == 0 gives num == 0: s* = 0, the row itself)
      const double s = num / dd;
      const double qx = fma(s, dx, p0x), qy = fma(s, dy, p0y);
      const double q2 = fma(qx, qx, qy * qy), u = ui + s;
      if (aud_less(q2, u, j, bd2, bu, bj)) { bd2 = q2; bu = u; bj = j; }
    }
  }
  return r2;
}
