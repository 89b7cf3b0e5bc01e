// d2d_fleet_audit: the closest approach of every aircraft to the aircraft of OTHER formations in its world, continuous in time between
// rows, through a spatial broad phase (include/d2d.h states the call; tests/fleet_audit_ref.py is the CPU statement, brute force).
//
// The candidates and their keys are aud_segment's (audit_device.h), the sequence the in-formation audit compiles.  A candidate counts
// only below d_look, so the answer is a property of the history; the grid only decides which pairs are looked at, and it looks at
// every pair that can count: cells of edge (d_look + 2 step_max)(1 + 2^-16), every aircraft binned at every row, a query over the 3 x 3
// cells around its own cell at the segment's first row (the argument, roundings included, is in include/d2d.h).
//
// The refusal pass, the formation table, the bin pass and the parameter rules live in fleet_device.h, which d2d_fleet_tracks
// (fleet_tracks.hip) includes too.
// Kernels.  fleet_check_kernel: lanes along the drone index, the rows cut into FLT_CHECK_BLOCKS blocks; every (lane, block) stores the
// refusal bits of its own rows -- one word, one owner -- and block 0 resets the aircraft's running key.  fleet_meta_kernel: a lane per
// formation ORs its aircraft's words, adds the row0 rule and writes the status and the formation's (row0, valid rows, world), the
// valid rows of a refused formation as 0: it is never binned and never asked for, which is all that "invisible" takes.
// Then per tile of tile_rows global rows: the list heads are set to -1; fleet_bin_kernel, a lane per (aircraft, row), pushes the
// aircraft on the list of the slot of its (world, cell) with one integer exchange on the head, the old head its `next` (the only
// atomic of the call; the kernel boundary publishes the lists), and stores its node: positions, formation, world.
// fleet_query_kernel, a lane per (aircraft, row), walks the lists of the distinct slots of its nine cells, skips its own formation
// and other worlds, and stores the key and the count flag of that row.  fleet_fold_kernel, a lane per aircraft, folds the tile's
// rows into the running key.  A list holds whatever shares the slot (other
// cells, other worlds): that costs a look, and a list's order is not seen, since the fold is a minimum of keys.
// fleet_final_kernel: a lane per aircraft draws the root and writes the outputs.  No floating-point atomic, no floating-point sum.
#include "fleet_device.h"

namespace {

struct FleetArgs : FleetCore {
  double *kd2, *ku;                  // [N] the running key ...
  int32_t *kj, *kcnt;                // ... its partner, and the count
  double *td2, *tu;                 // [tile][N] the key of a row
  int32_t *tj;                       // [tile][N] its partner, -1: nothing seen at that row
  int32_t *tc;                       // [tile][N] 1 when the row counts against d_safe
  d2d_fleet_out out;
};

__global__ void __launch_bounds__(FLT_WG)
fleet_check_kernel(FleetArgs A) {
  const int d = blockIdx.x * FLT_WG + threadIdx.x, b = blockIdx.y;
  if (d >= A.N) return;
  flt_check_rows(A, d, b);
  if (b == 0) { A.kd2[d] = A.look2; A.ku[d] = -aud_inf(); A.kj[d] = -1; A.kcnt[d] = 0; }     // below every key that counts: d2 < look2
}

__global__ void __launch_bounds__(FLT_WG)
fleet_query_kernel(FleetArgs A, int g0, int n_tile) {
  int bx, r;
  if (!flt_block(A.wgx, n_tile, bx, r)) return;
  const int d = bx * FLT_WG + threadIdx.x, N = A.N;
  if (d >= N) return;
  const int f = d / A.p.n_ac, g = g0 + r;
  const int4 m = A.meta[f];
  const int i = g - m.x;
  double bd2 = A.look2, bu = -aud_inf(); int bj = -1, cnt = 0;
  if (i >= 0 && i < m.y) {
    const bool seg_own = i + 1 < m.y;
    const double cx = flt_plane(A.X, N, i, 0)[d], cy = flt_plane(A.X, N, i, 1)[d];
    double nx = 0, ny = 0;
    if (seg_own) { nx = flt_plane(A.X, N, i + 1, 0)[d]; ny = flt_plane(A.X, N, i + 1, 1)[d]; }
    const int ix = flt_cell(cx, A.inv_edge), iy = flt_cell(cy, A.inv_edge);
    const unsigned mask = (unsigned)A.slots - 1u;
    const int32_t *heads = A.heads + (size_t)r * A.slots;
    const FleetNode *node = A.node + (size_t)r * N;
    unsigned seen[9];
    double rmin = aud_inf();
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const unsigned s = flt_slot(m.z, ix + c % 3 - 1, iy + c / 3 - 1, mask);
      seen[c] = s;
      bool again = false;
#pragma unroll
      for (int k = 0; k < c; ++k) again |= seen[k] == s;     // two cells on one slot: the list is walked once
      if (again) continue;
      for (int e = heads[s]; e >= 0;) {
        const FleetNode n = node[e];                         // valid at g: it is on this row's list
        if (n.form != f && n.world == m.z)
          rmin = fmin(rmin, aud_segment(n.x0 - cx, n.y0 - cy, n.x1 - nx, n.y1 - ny, seg_own && n.seg, g, e, bd2, bu, bj));
        e = n.next;
      }
    }
    cnt = rmin < A.safe2;
  }
  const size_t o = (size_t)r * N + d;
  A.td2[o] = bd2; A.tu[o] = bu; A.tj[o] = bj; A.tc[o] = cnt;
}

__global__ void __launch_bounds__(FLT_WG)
fleet_fold_kernel(FleetArgs A, int n_tile) {
  const int d = blockIdx.x * FLT_WG + threadIdx.x, N = A.N;
  if (d >= N) return;
  double bd2 = A.kd2[d], bu = A.ku[d]; int bj = A.kj[d], cnt = A.kcnt[d];
  for (int r = 0; r < n_tile; ++r) {
    const size_t o = (size_t)r * N + d;
    const double d2 = A.td2[o], u = A.tu[o];
    const int j = A.tj[o];
    cnt += A.tc[o];
    if (j >= 0 && aud_less(d2, u, j, bd2, bu, bj)) { bd2 = d2; bu = u; bj = j; }
  }
  A.kd2[d] = bd2; A.ku[d] = bu; A.kj[d] = bj; A.kcnt[d] = cnt;
}

__global__ void __launch_bounds__(FLT_WG)
fleet_final_kernel(FleetArgs A) {
  const int d = blockIdx.x * FLT_WG + threadIdx.x;
  if (d >= A.N) return;
  const int f = d / A.p.n_ac, status = A.meta[f].w;
  if (A.out.status && d % A.p.n_ac == 0) A.out.status[f] = status;
  const bool ok = status == 0;
  const int bj = A.kj[d];
  const double nan = aud_nan();
  if (A.out.near_dist) A.out.near_dist[d] = ok ? (bj >= 0 ? sqrt(A.kd2[d]) : aud_inf()) : nan;
  if (A.out.near_time) A.out.near_time[d] = ok && bj >= 0 ? A.ku[d] * A.p.dt_row : nan;
  if (A.out.near_partner) A.out.near_partner[d] = ok ? bj : -1;
  if (A.out.near_count) A.out.near_count[d] = ok ? A.kcnt[d] : -1;
}

// the workspace's parts in order; returns its size (base NULL: the size alone)
size_t fleet_carve(FleetArgs &A, char *base) {
  FleetCarver c{base};
  const size_t N = (size_t)A.N, T = (size_t)A.tile;
  A.meta = c.take<int4>((size_t)A.p.n_form);
  A.dbad = c.take<int32_t>(FLT_CHECK_BLOCKS * N);
  A.kd2 = c.take<double>(N);
  A.ku = c.take<double>(N);
  A.kj = c.take<int32_t>(N);
  A.kcnt = c.take<int32_t>(N);
  A.heads = c.take<int32_t>(T * (size_t)A.slots);
  A.node = c.take<FleetNode>(T * N);
  A.td2 = c.take<double>(T * N);
  A.tu = c.take<double>(T * N);
  A.tj = c.take<int32_t>(T * N);
  A.tc = c.take<int32_t>(T * N);
  return c.off;
}

}  // namespace

extern "C" {

int64_t d2d_fleet_audit_workspace(const d2d_fleet_params *p) {
  FleetArgs A{};
  if (fleet_plan(p, "d2d_fleet_audit_workspace", A)) return D2D_EINVAL;
  return (int64_t)fleet_carve(A, nullptr);
}

int d2d_fleet_audit(d2d_ctx *ctx, const d2d_fleet_params *p, const double *X_hist, const int32_t *rows, const int32_t *row0,
                    const int32_t *world, void *work, const d2d_fleet_out *out) {
  D2D_REQUIRE(ctx && X_hist && out && work, "d2d_fleet_audit: null argument (ctx, X_hist, work or out)");
  FleetArgs A{};
  if (int rc = fleet_plan(p, "d2d_fleet_audit", A)) return rc;
  fleet_carve(A, static_cast<char *>(work));
  A.X = X_hist; A.rows = rows; A.row0 = row0; A.world = world; A.prio = nullptr; A.out = *out;
  const unsigned wgx = (unsigned)((A.N + FLT_WG - 1) / FLT_WG);
  A.wgx = (int)wgx;
  hipLaunchKernelGGL(fleet_check_kernel, dim3(wgx, FLT_CHECK_BLOCKS), dim3(FLT_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  hipLaunchKernelGGL(fleet_meta_kernel, dim3((unsigned)((p->n_form + FLT_WG - 1) / FLT_WG)), dim3(FLT_WG), 0, ctx->stream, (const FleetCore &)A);
  D2D_LAUNCH_CHECK();
  for (long long g0l = 0; g0l < p->g_rows; g0l += A.tile) {       // (64 bits: g_rows may be within a tile of 2^31)
    const int g0 = (int)g0l, n_tile = (int)std::min<long long>(A.tile, p->g_rows - g0l);
    D2D_CHECK_HIP(hipMemsetAsync(A.heads, 0xFF, (size_t)n_tile * A.slots * sizeof(int32_t), ctx->stream));      // every head -1
    const dim3 grid(wgx * (unsigned)((n_tile + 7) / 8 * 8));
    hipLaunchKernelGGL(fleet_bin_kernel, grid, dim3(FLT_WG), 0, ctx->stream, (const FleetCore &)A, g0, n_tile);
    D2D_LAUNCH_CHECK();
    hipLaunchKernelGGL(fleet_query_kernel, grid, dim3(FLT_WG), 0, ctx->stream, A, g0, n_tile);
    D2D_LAUNCH_CHECK();
    hipLaunchKernelGGL(fleet_fold_kernel, dim3(wgx), dim3(FLT_WG), 0, ctx->stream, A, n_tile);
    D2D_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fleet_final_kernel, dim3(wgx), dim3(FLT_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  return D2D_OK;
}

}  // extern "C"
