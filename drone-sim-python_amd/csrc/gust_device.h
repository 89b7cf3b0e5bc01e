// Stochastic gusts of the plant (include/d2d.h d2d_gust): Philox4x32-10, the normal pair of a step and the first-order
// Gauss-Markov state update.  Every number is a function of (seed, stream, phase, part, step) and of the lane's own state: no wave
// vote, no exchange, no atomics -- a drone's gust does not depend on the batch, the block layout or the shard it is flown in.
// Every product that an addition follows is written as fma: the sample kernel and the time loops then round alike whatever the
// compiler would have contracted in their different surroundings.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/d2d.h"

struct Philox4 {
  uint32_t r[4];
};

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl increments between them.  The 32 x 32 -> 64 products
// are plain 64-bit multiplications.
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

struct Normal2 {
  double x, y;
};

// The two standard normals of (stream, sub, step): one Philox call, two 53-bit uniforms in (0, 1) (exact in fp64), Box-Muller.
__device__ __forceinline__ Normal2 gust_normals(uint64_t seed, uint64_t stream, uint32_t sub, uint32_t step) {
  const Philox4 q = philox4x32_10(step, (uint32_t)stream, (uint32_t)(stream >> 32), sub, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u1 = ((double)(q.r[0] >> 5) * 67108864.0 + ((double)(q.r[1] >> 6) + 0.5)) * 0x1p-53;
  const double u2 = ((double)(q.r[2] >> 5) * 67108864.0 + ((double)(q.r[3] >> 6) + 0.5)) * 0x1p-53;
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  return {rad * cs, rad * sn};
}

// The lane's gust: its own process o, its formation's shared process h (the same numbers on every aircraft of the formation) and
// the two stream words they draw on.
struct GustState {
  double ox, oy, hx, hy;
  uint64_t own, form;
};

// drone d of N: o_0 from state_in or, without one, the stationary start sigma xi(step_base).  (The 64-bit division by n_ac is paid
// here, once per lane.)
__device__ __forceinline__ GustState gust_begin(const d2d_gust &g, long d, long N) {
  GustState st;
  st.own = (uint64_t)(g.stream_base + d);
  st.form = st.own / (uint64_t)g.n_ac;
  st.hx = 0.0; st.hy = 0.0;
  if (g.state_in) {
    st.ox = g.state_in[d]; st.oy = g.state_in[N + d]; st.hx = g.state_in[2 * N + d]; st.hy = g.state_in[3 * N + d];
  } else {
    const Normal2 n = gust_normals((uint64_t)g.seed, st.own, 2u * (uint32_t)g.phase, (uint32_t)g.step_base);
    st.ox = g.sigma * n.x; st.oy = g.sigma * n.y;
    if (g.w_form != 0.0) {
      const Normal2 m = gust_normals((uint64_t)g.seed, st.form, 2u * (uint32_t)g.phase + 1u, (uint32_t)g.step_base);
      st.hx = g.sigma * m.x; st.hy = g.sigma * m.y;
    }
  }
  return st;
}

// g = w_own o + w_form h
__device__ __forceinline__ Normal2 gust_value(const d2d_gust &g, const GustState &st) {
  return {fma(g.w_own, st.ox, g.w_form * st.hx), fma(g.w_own, st.oy, g.w_form * st.hy)};
}

// o_i = a o_{i-1} + s xi_i with the draw at counter step_base + i; without a shared part its call is not made (wave-uniform)
__device__ __forceinline__ void gust_advance(const d2d_gust &g, GustState &st, int i) {
  const uint32_t step = (uint32_t)g.step_base + (uint32_t)i;
  const Normal2 n = gust_normals((uint64_t)g.seed, st.own, 2u * (uint32_t)g.phase, step);
  st.ox = fma(g.a, st.ox, g.s * n.x); st.oy = fma(g.a, st.oy, g.s * n.y);
  if (g.w_form != 0.0) {
    const Normal2 m = gust_normals((uint64_t)g.seed, st.form, 2u * (uint32_t)g.phase + 1u, step);
    st.hx = fma(g.a, st.hx, g.s * m.x); st.hy = fma(g.a, st.hy, g.s * m.y);
  }
}

__device__ __forceinline__ void gust_store_state(const d2d_gust &g, const GustState &st, long d, long N) {
  if (g.state_out) {
    g.state_out[d] = st.ox; g.state_out[N + d] = st.oy; g.state_out[2 * N + d] = st.hx; g.state_out[3 * N + d] = st.hy;
  }
}

__device__ __forceinline__ void gust_store_row(const d2d_gust &g, const GustState &st, long row, long d, long N) {
  if (g.g_hist) {
    const Normal2 v = gust_value(g, st);
    g.g_hist[row * 2 * N + d] = v.x; g.g_hist[row * 2 * N + N + d] = v.y;
  }
}
