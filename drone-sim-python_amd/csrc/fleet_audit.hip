// d2d_fleet_audit: the closest approach of every aircraft to the aircraft of OTHER formations in its world, continuous in time between
// rows, through a spatial broad phase (include/d2d.h states the call; tests/fleet_audit_ref.py is the CPU statement, brute force).
//
// The candidates and their keys are aud_segment's (audit_device.h), the sequence the in-formation audit compiles.  A candidate counts
// only below d_look, so the answer is a property of the history; the grid only decides which pairs are looked at, and it looks at
// every pair that can count: cells of edge (d_look + 2 step_max)(1 + 2^-16), every aircraft binned at every row, a query over the 3 x 3
// cells around its own cell at the segment's first row (the argument, roundings included, is in include/d2d.h).
//
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
#include "common.h"
#include "audit_device.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int FLT_WG = 256;
constexpr int FLT_CHECK_BLOCKS = 8;          // row blocks of the check pass (its words: FLT_CHECK_BLOCKS * N)
constexpr int FLT_MAX_TILE = 32768;          // rows of a tile at most
constexpr int FLT_MAX_SLOTS = 1 << 24;
constexpr long long FLT_TILE_LANES = 1 << 20;  // the library's tile: about this many (aircraft, row) lanes per launch ...
constexpr int FLT_TILE_LO = 4, FLT_TILE_HI = 64;   // ... within these bounds
constexpr double FLT_EDGE_MARGIN = 1.0 / 65536.0;  // relative inflation of the cell edge (include/d2d.h: why no pair is lost)
constexpr double FLT_CELL_MAX = 1073741824.0;      // |coordinate / edge| beyond 2^30: D2D_FLEET_RANGE

// What a list walk reads of an aircraft at a binned row, in ONE 64-byte line: a walk is a chain of dependent gathers, and reading
// the positions from the history planes and the formation's clock and world from their tables costs six lines per entry instead.
struct alignas(16) FleetNode {         // (the workspace is promised 16-byte aligned; its parts are cut at multiples of 64)
  double x0, y0, x1, y1;             // the position at the row and, with seg, at the next row (the history's own values)
  int32_t next, form, world, seg;    // the next aircraft of the slot's list (-1: none); its formation and world; valid at the next row
  int32_t pad[4];
};
static_assert(sizeof(FleetNode) == 64, "a node is one line");

struct FleetArgs {
  d2d_fleet_params p;
  int N, tile, slots, wgx;           // wgx: workgroups along the drone index
  double inv_edge, look2, safe2, step2;
  const double *X;
  const int32_t *rows, *row0, *world;
  int32_t *dbad;                     // [FLT_CHECK_BLOCKS][N] refusal bits of a drone's rows in a block
  int4 *meta;                        // [n_form] (row0, valid rows -- both 0 when refused --, world, status)
  double *kd2, *ku;                  // [N] the running key ...
  int32_t *kj, *kcnt;                // ... its partner, and the count
  int32_t *heads;                    // [tile][slots] the first aircraft of a slot's list, -1: empty
  FleetNode *node;                   // [tile][N] an aircraft at a row, as a list walk needs it
  double *td2, *tu;                  // [tile][N] the key of a row
  int32_t *tj;                       // [tile][N] its partner, -1: nothing seen at that row
  int32_t *tc;                       // [tile][N] 1 when the row counts against d_safe
  d2d_fleet_out out;
};

__device__ __forceinline__ const double *flt_plane(const double *X, int N, int row, int plane) {
  return X + ((size_t)row * 5 + plane) * (size_t)N;
}

__device__ __forceinline__ int flt_rows(const FleetArgs &A, int f) {
  return A.rows ? min(max(A.rows[f], 0), A.p.n_rows) : A.p.n_rows;
}

// cell index of a coordinate of a non-refused formation: |x * inv_edge| <= 2^30, so the conversion is exact and +-1 cannot wrap
__device__ __forceinline__ int flt_cell(double x, double inv_edge) { return (int)floor(x * inv_edge); }

// The slot of a cell: eight cells that are neighbours along x share one hashed group of eight consecutive heads (32 bytes), so the
// three heads of a row of the 3 x 3 cells come with one or two memory lines instead of three.
__device__ __forceinline__ unsigned flt_slot(int world, int cx, int cy, unsigned mask) {
  unsigned h = (unsigned)(cx >> 3) * 0x9E3779B1u ^ (unsigned)cy * 0x85EBCA77u ^ (unsigned)world * 0xC2B2AE3Du;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  return (h << 3 | ((unsigned)cx & 7u)) & mask;
}

// The (aircraft block, row) of a workgroup of the bin and query launches.  Workgroups are dealt round-robin over the eight XCDs, so
// workgroup id & 7 picks the row within a group of eight rows and the rest walks the aircraft: the workgroups that share an L2 then
// work on ONE row's heads and nodes (4 MiB of nodes per 65 536 aircraft) instead of on every row in flight.  For speed only: any
// placement gives the same result.  False: a row past the tile's end.
__device__ __forceinline__ bool flt_block(int wgx, int n_tile, int &bx, int &r) {
  const int id = blockIdx.x, chunk = id >> 3;
  bx = chunk % wgx;
  r = (chunk / wgx) * 8 + (id & 7);
  return r < n_tile;
}

__global__ void __launch_bounds__(FLT_WG)
fleet_check_kernel(FleetArgs A) {
  const int d = blockIdx.x * FLT_WG + threadIdx.x, b = blockIdx.y, N = A.N;
  if (d >= N) return;
  const int rows_f = flt_rows(A, d / A.p.n_ac);
  const int rpb = (A.p.n_rows + FLT_CHECK_BLOCKS - 1) / FLT_CHECK_BLOCKS;
  const int i0 = b * rpb, i1 = min(i0 + rpb, rows_f);
  int bad = 0;
  if (i0 < i1) {
    double cx = flt_plane(A.X, N, i0, 0)[d], cy = flt_plane(A.X, N, i0, 1)[d];
    for (int i = i0; i < i1; ++i) {
      if (!aud_finite(cx) || !aud_finite(cy)) bad |= D2D_FLEET_NONFINITE;
      if (fabs(cx * A.inv_edge) > FLT_CELL_MAX || fabs(cy * A.inv_edge) > FLT_CELL_MAX) bad |= D2D_FLEET_RANGE;
      if (i + 1 < rows_f) {              // the step that leaves the block's last row is this block's
        const double nx = flt_plane(A.X, N, i + 1, 0)[d], ny = flt_plane(A.X, N, i + 1, 1)[d];
        const double dx = nx - cx, dy = ny - cy;
        if (fma(dx, dx, dy * dy) > A.step2) bad |= D2D_FLEET_STEP;
        cx = nx; cy = ny;
      }
    }
  }
  A.dbad[(size_t)b * N + d] = bad;
  if (b == 0) { A.kd2[d] = A.look2; A.ku[d] = -aud_inf(); A.kj[d] = -1; A.kcnt[d] = 0; }     // below every key that counts: d2 < look2
}

__global__ void __launch_bounds__(FLT_WG)
fleet_meta_kernel(FleetArgs A) {
  const int f = blockIdx.x * FLT_WG + threadIdx.x;
  if (f >= A.p.n_form) return;
  const int n_ac = A.p.n_ac, rows_f = flt_rows(A, f), r0 = A.row0 ? A.row0[f] : 0;
  int status = 0;
  for (int b = 0; b < FLT_CHECK_BLOCKS; ++b)
    for (int a = 0; a < n_ac; ++a) status |= A.dbad[(size_t)b * A.N + (size_t)f * n_ac + a];
  if (r0 < 0 || (long long)r0 + rows_f > (long long)A.p.g_rows) status |= D2D_FLEET_BAD_ROW0;
  A.meta[f] = make_int4(status ? 0 : r0, status ? 0 : rows_f, A.world ? A.world[f] : 0, status);
}

__global__ void __launch_bounds__(FLT_WG)
fleet_bin_kernel(FleetArgs A, int g0, int n_tile) {
  int bx, r;
  if (!flt_block(A.wgx, n_tile, bx, r)) return;
  const int d = bx * FLT_WG + threadIdx.x, N = A.N;
  if (d >= N) return;
  const int4 m = A.meta[d / A.p.n_ac];
  const int i = g0 + r - m.x;
  if (i < 0 || i >= m.y) return;                       // not valid at this global row (m.y = 0: refused)
  const double x = flt_plane(A.X, N, i, 0)[d], y = flt_plane(A.X, N, i, 1)[d];
  const unsigned s = flt_slot(m.z, flt_cell(x, A.inv_edge), flt_cell(y, A.inv_edge), (unsigned)A.slots - 1u);
  FleetNode n;
  n.x0 = x; n.y0 = y; n.x1 = n.y1 = 0.0; n.pad[0] = n.pad[1] = n.pad[2] = n.pad[3] = 0;
  n.form = d / A.p.n_ac; n.world = m.z; n.seg = i + 1 < m.y;
  if (n.seg) { n.x1 = flt_plane(A.X, N, i + 1, 0)[d]; n.y1 = flt_plane(A.X, N, i + 1, 1)[d]; }
  n.next = atomicExch(A.heads + (size_t)r * A.slots + s, d);
  A.node[(size_t)r * N + d] = n;
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

bool flt_pos_finite(double v) { return v > 0.0 && std::isfinite(v); }

// what makes the parameters D2D_EINVAL (include/d2d.h), and the geometry they give
int fleet_plan(const d2d_fleet_params *p, const char *who, FleetArgs &A) {
  D2D_REQUIRE(p, "%s: null parameters", who);
  D2D_REQUIRE(p->n_form >= 1 && p->n_ac >= 1 && p->n_ac <= 64, "%s: n_form >= 1 and n_ac in 1 .. 64 required (n_form=%d n_ac=%d)", who, p->n_form, p->n_ac);
  D2D_REQUIRE(p->n_rows >= 1 && p->g_rows >= 1, "%s: n_rows >= 1 and g_rows >= 1 required (n_rows=%d g_rows=%d)", who, p->n_rows, p->g_rows);
  D2D_REQUIRE(flt_pos_finite(p->dt_row) && flt_pos_finite(p->d_look) && flt_pos_finite(p->step_max),
              "%s: dt_row, d_look and step_max must be > 0 and finite (%g, %g, %g)", who, p->dt_row, p->d_look, p->step_max);
  D2D_REQUIRE(p->d_safe <= p->d_look, "%s: d_safe = %g > d_look = %g (the grid sees nothing beyond d_look)", who, p->d_safe, p->d_look);
  D2D_REQUIRE(p->tile_rows >= 0 && p->slots >= 0, "%s: tile_rows = %d, slots = %d (0: the library's choice)", who, p->tile_rows, p->slots);
  const long long N = (long long)p->n_form * p->n_ac;
  D2D_REQUIRE(N * 5 * (long long)p->n_rows < (1LL << 40) && N < (1LL << 31), "%s: history too large", who);
  A.p = *p; A.N = (int)N;
  long long tile = p->tile_rows;
  if (tile == 0) tile = std::min<long long>(FLT_TILE_HI, std::max<long long>(FLT_TILE_LO, FLT_TILE_LANES / N));
  A.tile = (int)std::min<long long>(tile, FLT_MAX_TILE);    // (not cut to g_rows: the workspace is a function of N, tile_rows and slots alone)
  D2D_REQUIRE(N * (A.tile + 8LL) < (1LL << 31), "%s: tile_rows = %d with %lld drones: tile too large", who, p->tile_rows, N);
  long long want = p->slots == 0 ? 2 * N : p->slots;      // about two heads per aircraft of a row
  int slots = 1;
  while (slots < want && slots < FLT_MAX_SLOTS) slots *= 2;
  A.slots = slots;
  const double edge = (p->d_look + 2.0 * p->step_max) * (1.0 + FLT_EDGE_MARGIN);
  A.inv_edge = 1.0 / edge;
  A.look2 = p->d_look * p->d_look;
  A.safe2 = p->d_safe > 0.0 ? p->d_safe * p->d_safe : 0.0;
  A.step2 = p->step_max * p->step_max;
  return D2D_OK;
}

size_t up64(size_t n) { return (n + 63) / 64 * 64; }

// the workspace's parts in order; returns its size (base NULL: the size alone)
size_t fleet_carve(FleetArgs &A, char *base) {
  size_t off = 0;
  auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += up64(bytes); return q; };
  const size_t N = (size_t)A.N, T = (size_t)A.tile;
  A.meta = reinterpret_cast<int4 *>(take((size_t)A.p.n_form * sizeof(int4)));
  A.dbad = reinterpret_cast<int32_t *>(take(FLT_CHECK_BLOCKS * N * sizeof(int32_t)));
  A.kd2 = reinterpret_cast<double *>(take(N * sizeof(double)));
  A.ku = reinterpret_cast<double *>(take(N * sizeof(double)));
  A.kj = reinterpret_cast<int32_t *>(take(N * sizeof(int32_t)));
  A.kcnt = reinterpret_cast<int32_t *>(take(N * sizeof(int32_t)));
  A.heads = reinterpret_cast<int32_t *>(take(T * (size_t)A.slots * sizeof(int32_t)));
  A.node = reinterpret_cast<FleetNode *>(take(T * N * sizeof(FleetNode)));
  A.td2 = reinterpret_cast<double *>(take(T * N * sizeof(double)));
  A.tu = reinterpret_cast<double *>(take(T * N * sizeof(double)));
  A.tj = reinterpret_cast<int32_t *>(take(T * N * sizeof(int32_t)));
  A.tc = reinterpret_cast<int32_t *>(take(T * N * sizeof(int32_t)));
  return off;
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
  A.X = X_hist; A.rows = rows; A.row0 = row0; A.world = world; A.out = *out;
  const unsigned wgx = (unsigned)((A.N + FLT_WG - 1) / FLT_WG);
  A.wgx = (int)wgx;
  hipLaunchKernelGGL(fleet_check_kernel, dim3(wgx, FLT_CHECK_BLOCKS), dim3(FLT_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  hipLaunchKernelGGL(fleet_meta_kernel, dim3((unsigned)((p->n_form + FLT_WG - 1) / FLT_WG)), dim3(FLT_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  for (long long g0l = 0; g0l < p->g_rows; g0l += A.tile) {       // (64 bits: g_rows may be within a tile of 2^31)
    const int g0 = (int)g0l, n_tile = (int)std::min<long long>(A.tile, p->g_rows - g0l);
    D2D_CHECK_HIP(hipMemsetAsync(A.heads, 0xFF, (size_t)n_tile * A.slots * sizeof(int32_t), ctx->stream));      // every head -1
    const dim3 grid(wgx * (unsigned)((n_tile + 7) / 8 * 8));
    hipLaunchKernelGGL(fleet_bin_kernel, grid, dim3(FLT_WG), 0, ctx->stream, A, g0, n_tile);
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
