// d2d_fleet_tracks: for every formation the nearest aircraft of formations that OUTRANK it, as the moving-obstacle tables of the
// collocation planner (include/d2d.h states the call; tests/fleet_tracks_ref.py is the CPU statement, brute force over all pairs).
//
// The candidates and their keys are aud_segment's (audit_device.h) and the grid, the check, meta and bin passes are the fleet audit's
// (fleet_device.h): the answer is a property of the history, the grid only schedules.  What is kept is not one key but a LIST: the
// CAP = n_mov + 1 smallest distinct partners, each with the minimum of its keys (d2, u, A, B), sorted.  Merging two such lists --
// insert every entry of one into the other, an entry of a partner that is already there replacing it only when its key is smaller --
// is commutative and associative, and a partner of the final list is never lost on the way: fewer than CAP partners have smaller final
// keys, so fewer than CAP can stand before it in any partial list.  Every output is therefore the same bytes for every tile_rows and
// slots.  No floating-point atomic, no floating-point sum.
//
// Kernels.  tracks_check_kernel, fleet_meta_kernel, fleet_bin_kernel: as in fleet_audit.hip (the node carries its formation's priority).
// tracks_query_kernel: a lane per (aircraft, chunk of TRK_CHUNK rows of the tile) walks the nine cells of each of its rows, skips its
// own formation, other worlds and every formation that does not outrank its own, and inserts what is below d_look into a sorted list
// it holds in registers across the chunk; it stores the list's length and only that many entries.  Almost every lane stores a 0.
// tracks_fold_kernel: a lane per aircraft merges the tile's chunks into the aircraft's running list; an aircraft whose chunks are all
// empty reads its lengths and returns.  tracks_final_kernel: ONE wavefront per formation (n_ac <= 64), a lane per aircraft, a
// butterfly of list merges over the lanes, after which every lane holds the formation's list; the lanes then share the outputs:
// slots, knots and, per slot, the rows of the chord error with an exact maximum over the lanes.
#include "fleet_device.h"

#include <climits>

namespace {

constexpr int TRK_CHUNK = 4;           // rows of a tile that one query lane walks with its list in registers
constexpr int TRK_WAVE = 64;

// A sorted list of distinct partners in registers (every index is a compile-time constant after unrolling).  WA: the key carries the
// aircraft A of the own formation (the fold over a formation); without it all entries are one aircraft's and A is not stored.
template <int CAP> struct TrkList {
  double d2[CAP], u[CAP];
  int j[CAP], a[CAP];                  // j = -1: empty (its d2 is +inf, so it sorts last)
};

template <int CAP, bool WA> __device__ __forceinline__ void trk_clear(TrkList<CAP> &L) {
#pragma unroll
  for (int k = 0; k < CAP; ++k) { L.d2[k] = aud_inf(); L.u[k] = aud_inf(); L.j[k] = -1; if (WA) L.a[k] = INT_MAX; }
}

// (d2, u, a, j) < (e2, eu, ea, ej)
template <bool WA> __device__ __forceinline__ bool trk_less(double d2, double u, int a, int j, double e2, double eu, int ea, int ej) {
  if (d2 != e2) return d2 < e2;
  if (u != eu) return u < eu;
  if (WA && a != ea) return a < ea;
  return j < ej;
}

// merge one entry into the list: one pass of compare and exchange; the old entry of the same partner ends the pass
template <int CAP, bool WA> __device__ __forceinline__ void trk_insert(TrkList<CAP> &L, double d2, double u, int a, int j) {
  const int jn = j;
  bool done = false, placed = false;
#pragma unroll
  for (int k = 0; k < CAP; ++k) {
    if (done) continue;
    const bool same = L.j[k] == jn;
    const bool lt = trk_less<WA>(d2, u, a, j, L.d2[k], L.u[k], WA ? L.a[k] : 0, L.j[k]);
    if (same && !placed && !lt) { done = true; continue; }        // the partner is there with a key that is not larger
    if (same || lt) {                    // same: the old entry leaves (the carried one takes its place); lt: exchange and carry on
      const double t2 = L.d2[k], tu = L.u[k]; const int tj = L.j[k], ta = WA ? L.a[k] : 0;
      L.d2[k] = d2; L.u[k] = u; L.j[k] = j; if (WA) L.a[k] = a;
      d2 = t2; u = tu; j = tj; a = ta;
      placed = true;
      if (same) done = true;
    }
  }
}

template <int CAP> __device__ __forceinline__ int trk_count(const TrkList<CAP> &L) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < CAP; ++k) c += L.j[k] >= 0;
  return c;
}

struct TrkArgs : FleetCore {
  int n_mov, n_knot, kind, n_chunk;    // n_chunk: chunks of a whole tile
  double r_disc, t0;
  int32_t *ccnt;                       // [n_chunk][N] the length of a chunk's list
  double *cd2, *cu;                    // [n_chunk][CAP][N] its entries ...
  int32_t *cj;                         // ... and their partners
  int32_t *rcnt;                       // [N] the running list of an aircraft
  double *rd2, *ru;                    // [CAP][N]
  int32_t *rj;
  d2d_tracks_out out;
};

__global__ void __launch_bounds__(FLT_WG)
tracks_check_kernel(TrkArgs A) {
  const int d = blockIdx.x * FLT_WG + threadIdx.x, b = blockIdx.y;
  if (d >= A.N) return;
  flt_check_rows(A, d, b);
  if (b == 0) A.rcnt[d] = 0;
}

// (prio, form) of a partner below that of the own formation: it outranks us, we give way
__device__ __forceinline__ bool trk_outranks(int prio, int form, int my_prio, int f) { return prio < my_prio || (prio == my_prio && form < f); }

template <int CAP> __global__ void __launch_bounds__(FLT_WG)
tracks_query_kernel(TrkArgs A, int g0, int n_tile) {
  const int bx = blockIdx.x % A.wgx, ch = blockIdx.x / A.wgx;
  const int d = bx * FLT_WG + threadIdx.x, N = A.N;
  if (d >= N) return;
  const int f = d / A.p.n_ac;
  const int4 m = A.meta[f];
  const int my_prio = A.prio ? A.prio[f] : f;
  const unsigned mask = (unsigned)A.slots - 1u;
  TrkList<CAP> L;
  trk_clear<CAP, false>(L);
  const int r1 = min(n_tile, (ch + 1) * TRK_CHUNK);
  for (int r = ch * TRK_CHUNK; r < r1; ++r) {
    const int g = g0 + r, i = g - m.x;
    if (i < 0 || i >= m.y) continue;
    const bool seg_own = i + 1 < m.y;
    const double cx = flt_plane(A.X, N, i, 0)[d], cy = flt_plane(A.X, N, i, 1)[d];
    double nx = 0, ny = 0;
    if (seg_own) { nx = flt_plane(A.X, N, i + 1, 0)[d]; ny = flt_plane(A.X, N, i + 1, 1)[d]; }
    const int ix = flt_cell(cx, A.inv_edge), iy = flt_cell(cy, A.inv_edge);
    const int32_t *heads = A.heads + (size_t)r * A.slots;
    const FleetNode *node = A.node + (size_t)r * N;
    unsigned seen[9];
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
        if (n.form != f && n.world == m.z && trk_outranks(n.prio, n.form, my_prio, f)) {
          double bd2 = A.look2, bu = -aud_inf(); int bj = -1;       // this partner's candidates of this segment alone, below d_look
          aud_segment(n.x0 - cx, n.y0 - cy, n.x1 - nx, n.y1 - ny, seg_own && n.seg, g, e, bd2, bu, bj);
          if (bj >= 0) trk_insert<CAP, false>(L, bd2, bu, 0, e);
        }
        e = n.next;
      }
    }
  }
  const int cnt = trk_count(L);
  A.ccnt[(size_t)ch * N + d] = cnt;
#pragma unroll
  for (int k = 0; k < CAP; ++k)
    if (k < cnt) {
      const size_t o = ((size_t)ch * CAP + k) * N + d;
      A.cd2[o] = L.d2[k]; A.cu[o] = L.u[k]; A.cj[o] = L.j[k];
    }
}

template <int CAP> __global__ void __launch_bounds__(FLT_WG)
tracks_fold_kernel(TrkArgs A, int n_tile) {
  const int d = blockIdx.x * FLT_WG + threadIdx.x, N = A.N;
  if (d >= N) return;
  const int n_ch = (n_tile + TRK_CHUNK - 1) / TRK_CHUNK;
  int any = 0;
  for (int ch = 0; ch < n_ch; ++ch) any |= A.ccnt[(size_t)ch * N + d];
  if (!any) return;
  TrkList<CAP> L;
  trk_clear<CAP, false>(L);
  const int rc = A.rcnt[d];
#pragma unroll
  for (int k = 0; k < CAP; ++k)
    if (k < rc) { const size_t o = (size_t)k * N + d; L.d2[k] = A.rd2[o]; L.u[k] = A.ru[o]; L.j[k] = A.rj[o]; }
  for (int ch = 0; ch < n_ch; ++ch) {
    const int c = A.ccnt[(size_t)ch * N + d];
    for (int k = 0; k < c; ++k) {
      const size_t o = ((size_t)ch * CAP + k) * N + d;
      trk_insert<CAP, false>(L, A.cd2[o], A.cu[o], 0, A.cj[o]);
    }
  }
  const int cnt = trk_count(L);
  A.rcnt[d] = cnt;
#pragma unroll
  for (int k = 0; k < CAP; ++k)
    if (k < cnt) { const size_t o = (size_t)k * N + d; A.rd2[o] = L.d2[k]; A.ru[o] = L.u[k]; A.rj[o] = L.j[k]; }
}

// entry m of a list whose index is not a compile-time constant
template <int CAP> __device__ __forceinline__ void trk_pick(const TrkList<CAP> &L, int m, double &d2, double &u, int &j) {
  d2 = aud_inf(); u = aud_inf(); j = -1;
#pragma unroll
  for (int k = 0; k < CAP; ++k)
    if (k == m) { d2 = L.d2[k]; u = L.u[k]; j = L.j[k]; }
}

// The global row of knot k of a formation with rows_f >= 2 valid rows from r0 (include/d2d.h), and the knot's time: the product
// rounded, then the sum rounded -- not fused, so that t0 + g * dt_row in any language states it.
__device__ __forceinline__ long long trk_knot_row(int r0, int rows_f, int n_knot, int k) {
  return (long long)r0 + ((long long)k * (rows_f - 1)) / (n_knot - 1);
}
__device__ __forceinline__ double trk_time(long long g, double dt_row, double t0) {
#pragma clang fp contract(off)
  const double p = (double)g * dt_row;
  return t0 + p;
}

// The squared distance between B's position (bx, by) at a row and the written track there: the track between its knots (x0, y0) and
// (x1, y1) at the fraction s.  Every operation rounded on its own (tests/fleet_tracks_ref.py chord_err states the sequence).
__device__ __forceinline__ double trk_chord2(double bx, double by, double x0, double y0, double x1, double y1, double s) {
#pragma clang fp contract(off)
  const double dx = x1 - x0, dy = y1 - y0;
  const double sx = s * dx, sy = s * dy;
  const double px = x0 + sx, py = y0 + sy;
  const double ex = bx - px, ey = by - py;
  const double exx = ex * ex, eyy = ey * ey;
  return exx + eyy;
}

template <int CAP> __global__ void __launch_bounds__(TRK_WAVE)
tracks_final_kernel(TrkArgs A) {
  const int f = blockIdx.x, lane = threadIdx.x, N = A.N, n_ac = A.p.n_ac;
  const int n_mov = A.n_mov, n_knot = A.n_knot;
  const int4 mf = A.meta[f];
  const int rows_f = flt_rows(A, f), r0 = A.row0 ? A.row0[f] : 0;
  const int status = mf.w | (rows_f < n_knot ? D2D_TRACKS_SHORT : 0);
  const bool ok = status == 0;
  TrkList<CAP> L;
  trk_clear<CAP, true>(L);
  if (ok && lane < n_ac) {
    const int d = f * n_ac + lane, rc = A.rcnt[d];
#pragma unroll
    for (int k = 0; k < CAP; ++k)
      if (k < rc) { const size_t o = (size_t)k * N + d; L.d2[k] = A.rd2[o]; L.u[k] = A.ru[o]; L.j[k] = A.rj[o]; L.a[k] = d; }
  }
  for (int off = TRK_WAVE / 2; off > 0; off >>= 1) {          // after the last exchange every lane holds the formation's list
    TrkList<CAP> T;
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
      T.d2[k] = __shfl_xor(L.d2[k], off, TRK_WAVE); T.u[k] = __shfl_xor(L.u[k], off, TRK_WAVE);
      T.j[k] = __shfl_xor(L.j[k], off, TRK_WAVE); T.a[k] = __shfl_xor(L.a[k], off, TRK_WAVE);
    }
#pragma unroll
    for (int k = 0; k < CAP; ++k)
      if (T.j[k] >= 0) trk_insert<CAP, true>(L, T.d2[k], T.u[k], T.a[k], T.j[k]);
  }
  const int cnt = trk_count(L);
  if (lane == 0) {
    if (A.out.status) A.out.status[f] = status;
    if (A.out.n_conf) A.out.n_conf[f] = ok ? min(cnt, n_mov + 1) : -1;
  }
  const double nan = aud_nan();
  if (lane < n_mov) {
    double d2, u; int j;
    trk_pick(L, lane, d2, u, j);
    const size_t o = (size_t)f * n_mov + lane;
    if (A.out.partner) A.out.partner[o] = j;
    if (A.out.part_dist) A.out.part_dist[o] = ok ? (j >= 0 ? sqrt(d2) : aud_inf()) : nan;
    if (A.out.part_time) A.out.part_time[o] = j >= 0 ? u * A.p.dt_row : nan;
    if (A.out.disc) { A.out.disc[o * 2] = j >= 0 ? A.r_disc : 0.0; A.out.disc[o * 2 + 1] = (double)A.kind; }
  }
  if (A.out.knots)
    for (int idx = lane; idx < n_mov * n_knot; idx += TRK_WAVE) {
      const int mi = idx / n_knot, k = idx % n_knot;
      double d2, u; int j;
      trk_pick(L, mi, d2, u, j);
      // a refused formation has no window to cut: its dummy tracks take one knot per row from row0, which increases strictly all the same
      const long long g = ok ? trk_knot_row(r0, rows_f, n_knot, k) : (long long)r0 + k;
      double x = 0.0, y = 0.0;
      if (j >= 0) {
        const int4 mb = A.meta[j / n_ac];
        const int ib = (int)min(max(g - mb.x, 0LL), (long long)mb.y - 1);      // held at its first or last row outside its own window
        x = flt_plane(A.X, N, ib, 0)[j]; y = flt_plane(A.X, N, ib, 1)[j];
      }
      double *kn = A.out.knots + ((size_t)f * n_mov * n_knot + idx) * 3;
      kn[0] = trk_time(g, A.p.dt_row, A.t0); kn[1] = x; kn[2] = y;
    }
  if (A.out.chord_err)
    for (int mi = 0; mi < n_mov; ++mi) {                       // (uniform over the wavefront: every lane holds the same list)
      double d2, u; int j;
      trk_pick(L, mi, d2, u, j);
      double worst = 0.0;
      if (j >= 0) {
        const int4 mb = A.meta[j / n_ac];
        for (int i = lane; i < rows_f; i += TRK_WAVE) {
          const long long g = (long long)r0 + i;
          const long long ib = g - mb.x;
          if (ib < 0 || ib >= mb.y) continue;                  // B has no row there
          int k = 0;
          while (k < n_knot - 2 && trk_knot_row(r0, rows_f, n_knot, k + 1) <= g) ++k;
          const long long ga = trk_knot_row(r0, rows_f, n_knot, k), gb = trk_knot_row(r0, rows_f, n_knot, k + 1);
          const int ia = (int)min(max(ga - mb.x, 0LL), (long long)mb.y - 1), ic = (int)min(max(gb - mb.x, 0LL), (long long)mb.y - 1);
          const double s = (double)(g - ga) / (double)(gb - ga);
          const double e2 = trk_chord2(flt_plane(A.X, N, (int)ib, 0)[j], flt_plane(A.X, N, (int)ib, 1)[j],
                                       flt_plane(A.X, N, ia, 0)[j], flt_plane(A.X, N, ia, 1)[j],
                                       flt_plane(A.X, N, ic, 0)[j], flt_plane(A.X, N, ic, 1)[j], s);
          worst = fmax(worst, e2);
        }
        for (int off = TRK_WAVE / 2; off > 0; off >>= 1) worst = fmax(worst, __shfl_xor(worst, off, TRK_WAVE));
      }
      if (lane == 0) A.out.chord_err[(size_t)f * n_mov + mi] = ok ? sqrt(worst) : nan;
    }
}

int tracks_cap(int n_mov) { return n_mov <= 1 ? 2 : n_mov <= 4 ? 5 : D2D_MAX_MOV + 1; }

int tracks_plan(const d2d_fleet_params *p, int n_mov, const char *who, TrkArgs &A) {
  if (int rc = fleet_plan(p, who, A)) return rc;
  D2D_REQUIRE(n_mov >= 1 && n_mov <= D2D_MAX_MOV, "%s: n_mov = %d outside 1 .. %d", who, n_mov, D2D_MAX_MOV);
  A.n_mov = n_mov;
  A.n_chunk = (A.tile + TRK_CHUNK - 1) / TRK_CHUNK;
  D2D_REQUIRE((long long)A.wgx * A.n_chunk < (1LL << 31), "%s: tile_rows = %d with %d drones: tile too large", who, p->tile_rows, A.N);
  return D2D_OK;
}

// the workspace's parts in order; returns its size (base NULL: the size alone)
size_t tracks_carve(TrkArgs &A, char *base) {
  FleetCarver c{base};
  const size_t N = (size_t)A.N, T = (size_t)A.tile, C = (size_t)A.n_chunk, K = (size_t)tracks_cap(A.n_mov);
  A.meta = c.take<int4>((size_t)A.p.n_form);
  A.dbad = c.take<int32_t>(FLT_CHECK_BLOCKS * N);
  A.heads = c.take<int32_t>(T * (size_t)A.slots);
  A.node = c.take<FleetNode>(T * N);
  A.ccnt = c.take<int32_t>(C * N);
  A.cd2 = c.take<double>(C * K * N);
  A.cu = c.take<double>(C * K * N);
  A.cj = c.take<int32_t>(C * K * N);
  A.rcnt = c.take<int32_t>(N);
  A.rd2 = c.take<double>(K * N);
  A.ru = c.take<double>(K * N);
  A.rj = c.take<int32_t>(K * N);
  return c.off;
}

template <int CAP> int tracks_launch(d2d_ctx *ctx, const TrkArgs &A) {
  const unsigned wgx = (unsigned)A.wgx;
  const int g_rows = A.p.g_rows;
  hipLaunchKernelGGL(tracks_check_kernel, dim3(wgx, FLT_CHECK_BLOCKS), dim3(FLT_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  hipLaunchKernelGGL(fleet_meta_kernel, dim3((unsigned)((A.p.n_form + FLT_WG - 1) / FLT_WG)), dim3(FLT_WG), 0, ctx->stream, (const FleetCore &)A);
  D2D_LAUNCH_CHECK();
  for (long long g0l = 0; g0l < g_rows; g0l += A.tile) {
    const int g0 = (int)g0l, n_tile = (int)std::min<long long>(A.tile, g_rows - g0l);
    D2D_CHECK_HIP(hipMemsetAsync(A.heads, 0xFF, (size_t)n_tile * A.slots * sizeof(int32_t), ctx->stream));      // every head -1
    hipLaunchKernelGGL(fleet_bin_kernel, dim3(wgx * (unsigned)((n_tile + 7) / 8 * 8)), dim3(FLT_WG), 0, ctx->stream, (const FleetCore &)A, g0, n_tile);
    D2D_LAUNCH_CHECK();
    const unsigned n_ch = (unsigned)((n_tile + TRK_CHUNK - 1) / TRK_CHUNK);
    hipLaunchKernelGGL(tracks_query_kernel<CAP>, dim3(wgx * n_ch), dim3(FLT_WG), 0, ctx->stream, A, g0, n_tile);
    D2D_LAUNCH_CHECK();
    hipLaunchKernelGGL(tracks_fold_kernel<CAP>, dim3(wgx), dim3(FLT_WG), 0, ctx->stream, A, n_tile);
    D2D_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(tracks_final_kernel<CAP>, dim3((unsigned)A.p.n_form), dim3(TRK_WAVE), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  return D2D_OK;
}

}  // namespace

extern "C" {

int64_t d2d_fleet_tracks_workspace(const d2d_fleet_params *p, int n_mov) {
  TrkArgs A{};
  if (tracks_plan(p, n_mov, "d2d_fleet_tracks_workspace", A)) return D2D_EINVAL;
  return (int64_t)tracks_carve(A, nullptr);
}

int d2d_fleet_tracks(d2d_ctx *ctx, const d2d_fleet_params *p, const double *X_hist, const int32_t *rows, const int32_t *row0,
                     const int32_t *world, const int32_t *prio, int n_mov, int n_knot, double r_disc, int kind, double t0, void *work,
                     const d2d_tracks_out *out) {
  D2D_REQUIRE(ctx && X_hist && out && work, "d2d_fleet_tracks: null argument (ctx, X_hist, work or out)");
  TrkArgs A{};
  if (int rc = tracks_plan(p, n_mov, "d2d_fleet_tracks", A)) return rc;
  D2D_REQUIRE(n_knot >= 2 && n_knot <= D2D_MOV_MAX_KNOT, "d2d_fleet_tracks: n_knot = %d outside 2 .. %d", n_knot, D2D_MOV_MAX_KNOT);
  D2D_REQUIRE(flt_pos_finite(r_disc) && (kind == 0 || kind == 1) && std::isfinite(t0),
              "d2d_fleet_tracks: r_disc > 0 and finite, kind 0 or 1 and a finite t0 required (%g, %d, %g)", r_disc, kind, t0);
  tracks_carve(A, static_cast<char *>(work));
  A.X = X_hist; A.rows = rows; A.row0 = row0; A.world = world; A.prio = prio; A.out = *out;
  A.n_knot = n_knot; A.kind = kind; A.r_disc = r_disc; A.t0 = t0;
  switch (tracks_cap(n_mov)) {
    case 2: return tracks_launch<2>(ctx, A);
    case 5: return tracks_launch<5>(ctx, A);
    default: return tracks_launch<D2D_MAX_MOV + 1>(ctx, A);
  }
}

}  // extern "C"
