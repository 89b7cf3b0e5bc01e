// What d2d_fleet_audit (fleet_audit.hip) and d2d_fleet_tracks (fleet_tracks.hip) share: the refusal pass over the history, the
// per-formation table, the hashed grid of one tile of rows and the parameter rules.  Each file includes this header and compiles
// its own copy of the three kernels (internal linkage); what they compute is stated in include/d2d.h and in fleet_audit.hip.
#pragma once
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
  int32_t prio, pad[3];              // its formation's priority (prio NULL: the formation index); only d2d_fleet_tracks reads it
};
static_assert(sizeof(FleetNode) == 64, "a node is one line");

// the part of a call's arguments that the shared passes read
struct FleetCore {
  d2d_fleet_params p;
  int N, tile, slots, wgx;           // wgx: workgroups along the drone index
  double inv_edge, look2, safe2, step2;
  const double *X;
  const int32_t *rows, *row0, *world, *prio;
  int32_t *dbad;                     // [FLT_CHECK_BLOCKS][N] refusal bits of a drone's rows in a block
  int4 *meta;                        // [n_form] (row0, valid rows -- both 0 when refused --, world, status)
  int32_t *heads;                    // [tile][slots] the first aircraft of a slot's list, -1: empty
  FleetNode *node;                   // [tile][N] an aircraft at a row, as a list walk needs it
};

__device__ __forceinline__ const double *flt_plane(const double *X, int N, int row, int plane) {
  return X + ((size_t)row * 5 + plane) * (size_t)N;
}

__device__ __forceinline__ int flt_rows(const FleetCore &A, int f) {
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

// the refusal bits of drone d's rows in row block b, stored in its own word
__device__ __forceinline__ void flt_check_rows(const FleetCore &A, int d, int b) {
  const int N = A.N;
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
}

__global__ void __launch_bounds__(FLT_WG)
fleet_meta_kernel(FleetCore A) {
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
fleet_bin_kernel(FleetCore A, int g0, int n_tile) {
  int bx, r;
  if (!flt_block(A.wgx, n_tile, bx, r)) return;
  const int d = bx * FLT_WG + threadIdx.x, N = A.N;
  if (d >= N) return;
  const int f = d / A.p.n_ac;
  const int4 m = A.meta[f];
  const int i = g0 + r - m.x;
  if (i < 0 || i >= m.y) return;                       // not valid at this global row (m.y = 0: refused)
  const double x = flt_plane(A.X, N, i, 0)[d], y = flt_plane(A.X, N, i, 1)[d];
  const unsigned s = flt_slot(m.z, flt_cell(x, A.inv_edge), flt_cell(y, A.inv_edge), (unsigned)A.slots - 1u);
  FleetNode n;
  n.x0 = x; n.y0 = y; n.x1 = n.y1 = 0.0; n.pad[0] = n.pad[1] = n.pad[2] = 0;
  n.form = f; n.world = m.z; n.seg = i + 1 < m.y;
  n.prio = A.prio ? A.prio[f] : f;
  if (n.seg) { n.x1 = flt_plane(A.X, N, i + 1, 0)[d]; n.y1 = flt_plane(A.X, N, i + 1, 1)[d]; }
  n.next = atomicExch(A.heads + (size_t)r * A.slots + s, d);
  A.node[(size_t)r * N + d] = n;
}

bool flt_pos_finite(double v) { return v > 0.0 && std::isfinite(v); }

// what makes the parameters D2D_EINVAL (include/d2d.h), and the geometry they give
int fleet_plan(const d2d_fleet_params *p, const char *who, FleetCore &A) {
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
  A.wgx = (int)((N + FLT_WG - 1) / FLT_WG);
  return D2D_OK;
}

size_t up64(size_t n) { return (n + 63) / 64 * 64; }

// cuts the parts of a workspace in order (base NULL: the sizes alone are added up)
struct FleetCarver {
  char *base; size_t off = 0;
  template <class T> T *take(size_t count) {
    char *q = base ? base + off : nullptr;
    off += up64(count * sizeof(T));
    return reinterpret_cast<T *>(q);
  }
};

}  // namespace
