// d2d_nlp_guess_dubins: the start of a collocation solve from a Dubins path, built on the device (include/d2d.h states the call and
// the rule; tests/nlp_guess_ref.py is the CPU statement, and this file follows it decision for decision and operation for operation).
//
// One problem per WAVEFRONT, problems handed out by a grid-stride loop.  What a problem decides once -- its row, the refusal, the
// shortest word at the preferred speed, the word that is filled -- every lane computes for itself from wave-uniform values (the row
// is read through a uniform index: scalar loads), so nothing has to be broadcast.  A round of the 64-section search is one evaluation
// of L* per lane (its own point of the bracket, all six words) and one ballot; the first sub-interval whose ends are on different
// sides is a bit trick on the ballot's mask, and the new bracket is recomputed by every lane from the uniform k.  The 24 trial radii
// of the loose bracket are 24 lanes of one more evaluation.  The fill runs with lane = node in strides of 64, so each of the five
// planes of W [B][5][N] is written in full lines.  No LDS, no atomics, one owner per output; lane 0 stores the per-problem outputs.
//
// Contraction into fused multiply-adds is off in this file: the statement is numpy, which rounds every product, and the search's
// points and the word lengths then differ from it only through the transcendentals.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "common.h"
#include "fit_device.h"      // scenario row columns (D2D_SC_*), FIT_G

#pragma clang fp contract(off)

namespace {

constexpr int GS_WG = 256, GS_WAVES = GS_WG / 64;
constexpr int GS_MAX_BLOCKS = 4096;
constexpr double GS_PI = 3.141592653589793, GS_TWO_PI = 2.0 * GS_PI;

struct GuessGeom {             // the two poses in the air frame
  double x0, y0, psi0, x1, y1, psi1;
  double s0, c0, s1, c1, dpsi;
};
struct GuessWord {             // the shortest admissible word at a radius: its length (+inf: none), index and segment lengths
  double len, l1, l2, l3;
  int word;
};

__device__ __forceinline__ double gs_inf() { return __builtin_inf(); }
__device__ __forceinline__ double gs_nan() { return __builtin_nan(""); }
__device__ __forceinline__ bool gs_finite(double x) { return fabs(x) <= DBL_MAX; }
__device__ __forceinline__ double gs_mod2pi(double x) {
  const double r = fmod(x, GS_TWO_PI);
  return r < 0.0 ? r + GS_TWO_PI : r;
}

// one candidate into the running best: admissible only if the net turning is psi1 - psi0; ties stay with the lower index (the words
// arrive in index order where they can tie: see gs_words)
__device__ __forceinline__ void gs_put(GuessWord &best, int w, bool ok, double rho, double t, double mid, double q, double net, double dpsi) {
  const double l1 = rho * t, l3 = rho * q;
  const double len = (l1 + mid) + l3;
  if (ok && fabs(net - dpsi) <= D2D_GUESS_TURN_TOL && (len < best.len || (len == best.len && w < best.word))) {
    best.len = len; best.word = w; best.l1 = l1; best.l2 = mid; best.l3 = l3;
  }
}

// L*(rho) and its word (tests/nlp_guess_ref.py words / lstar)
__device__ __forceinline__ GuessWord gs_words(const GuessGeom &g, double rho) {
  GuessWord best;
  best.len = gs_inf(); best.word = 6; best.l1 = best.l2 = best.l3 = 0.0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const double a = (w == 0 || w == 2) ? 1.0 : -1.0, b = (w == 0 || w == 3) ? 1.0 : -1.0;
    const double dx = (g.x1 - b * rho * g.s1) - (g.x0 - a * rho * g.s0);
    const double dy = (g.y1 + b * rho * g.c1) - (g.y0 + a * rho * g.c0);
    const double l2 = dx * dx + dy * dy;
    const double gam = atan2(dy, dx);
    if (w < 2) {                                       // L S L, R S R and the C C C word of the same centres (s = a)
      const double l = sqrt(l2);
      double t = gs_mod2pi(a * (gam - g.psi0)), q = gs_mod2pi(b * (g.psi1 - gam));
      gs_put(best, w, true, rho, t, l, q, a * t + b * q, g.dpsi);
      const double A = acos(fmin(l / (4.0 * rho), 1.0));
      const double chi1 = gam + a * A + a * (0.5 * GS_PI);
      const double chi2 = (gam + GS_PI - a * A) + a * (0.5 * GS_PI);
      const double m = GS_PI + 2.0 * A;
      t = gs_mod2pi(a * (chi1 - g.psi0)); q = gs_mod2pi(a * (g.psi1 - chi2));
      gs_put(best, w == 0 ? 5 : 4, l <= 4.0 * rho, rho, t, rho * m, q, a * ((t - m) + q), g.dpsi);
    } else {                                           // L S R, R S L
      const double p2 = l2 - 4.0 * rho * rho;
      const double p = sqrt(fmax(p2, 0.0));
      const double chi = gam + a * atan2(2.0 * rho, p);
      const double t = gs_mod2pi(a * (chi - g.psi0)), q = gs_mod2pi(b * (g.psi1 - chi));
      gs_put(best, w, p2 >= 0.0, rho, t, p, q, a * t + b * q, g.dpsi);
    }
  }
  if (best.word == 6) best.word = -1;
  return best;
}

// the pose a distance d along a segment of sign s (0: straight) that starts at (x, y, psi)
__device__ __forceinline__ void gs_advance(double x, double y, double psi, double sps, double cps, int s, double rho, double d,
                                           double &ox, double &oy, double &opsi) {
  if (s == 0) {
    ox = x + d * cps; oy = y + d * sps; opsi = psi + 0.0 * d;
  } else {
    const double sg = (double)s;
    double sn, cn;
    opsi = psi + sg * (d / rho);
    sincos(opsi, &sn, &cn);
    ox = x + sg * rho * (sn - sps); oy = y - sg * rho * (cn - cps);
  }
}

__device__ __forceinline__ void gs_signs(int word, int sg[3]) {      // WORD_SIGNS of the statement
  sg[0] = (word == 0 || word == 2 || word == 5) ? 1 : -1;
  sg[1] = word < 4 ? 0 : (word == 4 ? 1 : -1);
  sg[2] = (word == 0 || word == 3 || word == 5) ? 1 : -1;
}

struct GuessArgs {
  int B, N;
  double h, kappa;
  const double *scen, *bounds, *v_pref;
  double *W;
  d2d_nlp_guess_out out;
};

__device__ __forceinline__ void gs_store(const GuessArgs &A, int b, int lane, int status, int word, double v, double rho, double L, double t_nat) {
  if (lane != 0) return;
  if (A.out.status) A.out.status[b] = status;
  if (A.out.word) A.out.word[b] = word;
  if (A.out.v) A.out.v[b] = v;
  if (A.out.rho) A.out.rho[b] = rho;
  if (A.out.L) A.out.L[b] = L;
  if (A.out.t_nat) A.out.t_nat[b] = t_nat;
}

// ROUNDS rounds of 64-section on [a, b]: the side of the lower end is true and of the upper end false by the invariant.  tight: the
// unknown is the speed, side = F(v) > 0, and the result the last bracket's upper end; else the radius at the speed vp, side =
// L*(rho) - vp T < 0, and the result the lower end (the statement says why): the end where the path is no longer than v T.
__device__ __forceinline__ double gs_section(const GuessGeom &g, int lane, bool tight, double a, double b, double gt, double vp, double T) {
  for (int r = 0; r < D2D_GUESS_ROUNDS; ++r) {
    const double x = a + (b - a) * ((double)lane / 64.0);
    const double rho = tight ? x * x / gt : x;
    const double f = gs_words(g, rho).len - (tight ? x : vp) * T;
    const unsigned long long side = __ballot(tight ? f > 0.0 : f < 0.0) | 1ull;
    const int k = __ffsll((long long)(side & ~(side >> 1))) - 1;        // (bit 64, the upper end, is 0: side >> 1 brings it in)
    const double na = a + (b - a) * ((double)k / 64.0);
    if (k < 63) b = a + (b - a) * ((double)(k + 1) / 64.0);
    a = na;
  }
  return tight ? b : a;
}

__device__ __forceinline__ void gs_one(const GuessArgs &A, int b, int lane) {
  const int N = A.N;
  const double h = A.h;
  const double *sc = A.scen + (size_t)b * D2D_SCEN_STRIDE;
  const double x0 = sc[D2D_SC_X0], y0 = sc[D2D_SC_Y0], psi0 = sc[D2D_SC_PSI0], x1 = sc[D2D_SC_X1], y1 = sc[D2D_SC_Y1], psi1 = sc[D2D_SC_PSI1];
  const double wx = sc[D2D_SC_WX], wy = sc[D2D_SC_WY];         // the drift of the solver's equalities (nlp_constraint: - s.wx = + D2D_SC_WX)
  const double v_lo = sc[D2D_SC_VMIN], v_hi = sc[D2D_SC_VMAX];
  double phi_max = sc[D2D_SC_PHIMAX];
  bool fin = gs_finite(x0) && gs_finite(y0) && gs_finite(psi0) && gs_finite(x1) && gs_finite(y1) && gs_finite(psi1) && gs_finite(wx) && gs_finite(wy)
             && gs_finite(v_lo) && gs_finite(v_hi) && gs_finite(phi_max);
  if (A.bounds) {
    const double lo = A.bounds[(size_t)b * 4], hi = A.bounds[(size_t)b * 4 + 1];
    fin = fin && gs_finite(lo) && gs_finite(hi);
    if (lo < hi) phi_max = fmin(fabs(lo), fabs(hi));
  }
  double vp;
  if (A.v_pref) {
    vp = A.v_pref[b];
    fin = fin && gs_finite(vp);
  } else {
    const double kv = sc[D2D_SC_KV], vsp = sc[D2D_SC_VSP], vref = sc[D2D_SC_VREF];
    fin = fin && gs_finite(kv) && gs_finite(vsp) && gs_finite(vref);
    vp = kv > 0.0 ? vsp : (vref > 0.0 ? vref : 0.5 * (v_lo + v_hi));
  }
  if (!fin || !(v_lo > 0.0) || v_lo > v_hi || !(phi_max > 0.0 && phi_max < 0.5 * GS_PI)) {
    gs_store(A, b, lane, D2D_GUESS_INVALID, -1, gs_nan(), gs_nan(), gs_nan(), gs_nan());
    return;
  }
  vp = fmin(fmax(vp, v_lo), v_hi);
  const double T = (double)(N - 1) * h;
  GuessGeom g;
  g.x0 = x0; g.y0 = y0; g.psi0 = psi0; g.x1 = x1 - wx * T; g.y1 = y1 - wy * T; g.psi1 = psi1;
  sincos(psi0, &g.s0, &g.c0); sincos(psi1, &g.s1, &g.c1);
  g.dpsi = psi1 - psi0;
  const double gt = FIT_G * tan(A.kappa * phi_max);            // rho(v) = v^2 / gt
  const double rho0 = vp * vp / gt;
  const double L0 = gs_words(g, rho0).len;
  const double t_nat = gs_finite(L0) ? L0 / vp : gs_nan();
  bool line = fabs(g.dpsi) >= GS_TWO_PI || !gs_finite(L0) || L0 == 0.0;
  double v = vp, rho = rho0;
  int status = D2D_GUESS_LINE;
  if (!line) {
    if (L0 - vp * T > 0.0) {                                   // tight: a faster aircraft
      if (gs_words(g, v_hi * v_hi / gt).len - v_hi * T > 0.0) { v = v_hi; status = D2D_GUESS_SHORT; }
      else { v = gs_section(g, lane, true, vp, v_hi, gt, vp, T); status = D2D_GUESS_FIT; }
      rho = v * v / gt;
    } else {                                                   // loose: the preferred speed on wider turns
      double r = rho0;
      for (int i = 0; i < D2D_GUESS_GROW_MAX; ++i) if (i < lane) r *= D2D_GUESS_GROW;
      const bool reached = lane >= 1 && lane <= D2D_GUESS_GROW_MAX && gs_words(g, r).len - vp * T >= 0.0;
      const unsigned long long m = __ballot(reached);
      const int j = m ? __ffsll((long long)m) - 1 : D2D_GUESS_GROW_MAX;
      double lo = rho0, hi = rho0;
      for (int i = 0; i < j; ++i) { lo = hi; hi *= D2D_GUESS_GROW; }
      status = m ? D2D_GUESS_LOOSE : D2D_GUESS_LOOSE_UNMET;
      rho = m ? gs_section(g, lane, false, lo, hi, gt, vp, T) : hi;
    }
  }
  GuessWord ww;
  ww.len = gs_nan(); ww.word = -1; ww.l1 = ww.l2 = ww.l3 = 0.0;
  if (!line) {
    ww = gs_words(g, rho);
    line = !gs_finite(ww.len) || ww.len == 0.0;                // (a search that ended where no word is admissible)
  }
  double *Wb = A.W + (size_t)b * 5 * (size_t)N;
  const double den = (double)(N - 1);
  if (line) {
    const double dx = x1 - x0, dy = y1 - y0;
    for (int i = lane; i < N; i += 64) {
      const double frac = (double)i / den;
      const bool first = i == 0, last = i == N - 1;
      Wb[i] = first ? x0 : (last ? x1 : x0 + (x1 - x0) * frac);
      Wb[N + i] = first ? y0 : (last ? y1 : y0 + (y1 - y0) * frac);
      Wb[2 * N + i] = first ? psi0 : (last ? psi1 : psi0 + (psi1 - psi0) * frac);
      Wb[3 * N + i] = 0.0;
      Wb[4 * N + i] = vp;
    }
    gs_store(A, b, lane, D2D_GUESS_LINE, -1, vp, gs_inf(), sqrt(dx * dx + dy * dy), t_nat);
    return;
  }
  int sg[3];
  gs_signs(ww.word, sg);
  const double L = ww.len, l1 = ww.l1, l12 = ww.l1 + ww.l2;
  double px1, py1, pp1, px2, py2, pp2, sp1, cp1, sp2, cp2;
  gs_advance(x0, y0, psi0, g.s0, g.c0, sg[0], rho, l1, px1, py1, pp1);
  sincos(pp1, &sp1, &cp1);
  gs_advance(px1, py1, pp1, sp1, cp1, sg[1], rho, ww.l2, px2, py2, pp2);
  sincos(pp2, &sp2, &cp2);
  const double bank = atan(v * v / (FIT_G * rho));
  for (int i = lane; i < N; i += 64) {
    const double sig = i == N - 1 ? L : L * ((double)i / den);
    const int k = sig <= l1 ? 0 : (sig <= l12 ? 1 : 2);        // a node on a junction belongs to the earlier segment
    const double sx = k == 0 ? x0 : (k == 1 ? px1 : px2), sy = k == 0 ? y0 : (k == 1 ? py1 : py2), sp = k == 0 ? psi0 : (k == 1 ? pp1 : pp2);
    const double ss = k == 0 ? g.s0 : (k == 1 ? sp1 : sp2), cs = k == 0 ? g.c0 : (k == 1 ? cp1 : cp2);
    const double start = k == 0 ? 0.0 : (k == 1 ? l1 : l12);
    const int s = sg[k];
    double x, y, psi;
    gs_advance(sx, sy, sp, ss, cs, s, rho, sig - start, x, y, psi);
    const double t = (double)i * h;
    x = x + wx * t; y = y + wy * t;
    if (i == 0) { x = x0; y = y0; psi = psi0; }
    if (i == N - 1) { x = x1; y = y1; psi = psi1; }
    Wb[i] = x; Wb[N + i] = y; Wb[2 * N + i] = psi;
    Wb[3 * N + i] = (double)s * bank;
    Wb[4 * N + i] = v;
  }
  gs_store(A, b, lane, status, ww.word, v, rho, L, t_nat);
}

__global__ void __launch_bounds__(GS_WG)
nlp_guess_kernel(GuessArgs A) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * GS_WAVES + (threadIdx.x >> 6)));
  const int waves = (int)gridDim.x * GS_WAVES;
  for (int b = wave; b < A.B; b += waves) gs_one(A, b, lane);
}

}  // namespace

extern "C" {

int d2d_nlp_guess_dubins(d2d_ctx *ctx, int B, int N, double h, const double *scen, const d2d_nlp_guess_opts *opts, double *W,
                         const d2d_nlp_guess_out *out) {
  D2D_REQUIRE(ctx && scen && W, "d2d_nlp_guess_dubins: null argument (ctx, scen or W)");
  D2D_REQUIRE(B >= 1 && N >= 2 && h > 0 && std::isfinite(h), "d2d_nlp_guess_dubins: B >= 1, N >= 2, finite h > 0 required (B=%d N=%d h=%g)", B, N, h);
  GuessArgs A{};
  A.B = B; A.N = N; A.h = h; A.kappa = opts ? opts->kappa : D2D_GUESS_KAPPA;
  D2D_REQUIRE(A.kappa > 0.0 && A.kappa <= 1.0, "d2d_nlp_guess_dubins: kappa = %g outside (0, 1]", A.kappa);
  D2D_REQUIRE(!opts || opts->waves >= 0, "d2d_nlp_guess_dubins: waves = %d (0: the library's choice)", opts->waves);
  A.scen = scen; A.W = W;
  if (opts) { A.bounds = opts->bounds; A.v_pref = opts->v_pref; }
  if (out) A.out = *out;
  const long long want = opts && opts->waves > 0 ? opts->waves : B;
  const unsigned blocks = (unsigned)std::min<long long>((want + GS_WAVES - 1) / GS_WAVES, GS_MAX_BLOCKS);
  hipLaunchKernelGGL(nlp_guess_kernel, dim3(blocks), dim3(GS_WG), 0, ctx->stream, A);
  D2D_LAUNCH_CHECK();
  return D2D_OK;
}

}  // extern "C"
