// Device pieces of the input-gradient pass shared by k_sens.hip (reduction over the tower's input
// row) and k_macro_sens.hip (the state columns carried back through the LSTM): the LDS image, the
// W0^T fragments, the ReLU sign words and the per-tile forward / backward chain.
#pragma once
#include "common.h"
#include "layout.h"
#include "mlp.h"
#include "tower_dev.h"

// LDS image: [SDF fragments | aux | per-period inputs] (tower_dev.h, with blob_frags = m_fwd0),
// then the W0^T fragments (2 KS1 column blocks x 2 k-steps), then the wave-combine scratch.
__host__ __device__ inline size_t sens_w0t_base(const MlpDims& D) { return (lds_bytes_of(D) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t sens_red_base(const MlpDims& D, int KS1) {
  return sens_w0t_base(D) + (size_t)4 * KS1 * (D.fp32 ? 2048 : 1024);
}

// the launch's dims: only the SDF fragments [0, m_fwd0) of the blob are staged
inline MlpDims sens_dims(const MlpDims& D0) {
  MlpDims D = D0;
  D.blob_frags = D0.m_fwd0;
  return D;
}

// W0^T fragment (v, s): lane (q, n), element j = W0[unit 32s + perm(q, j)][panel column 16v + n]
template <class P, int KS1>
DLAP_DEV void build_w0t(typename P::Frag* w0t, const float* params, const PackLayer& L, const MlpDims& D) {
  const auto pg = gp(params);
  for (int f = threadIdx.x; f < 4 * KS1 * 64; f += blockDim.x) {
    const int frag = f >> 6, lane = f & 63, q = lane >> 4, n = lane & 15, v = frag >> 1, s = frag & 1;
    const int k = 16 * v + n;
    const int c = k < D.F ? k : (k >= D.ppc && k < D.ppc + D.Dm ? D.F + (k - D.ppc) : -1);
    typename P::Frag fr = P::zero();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int o = 32 * s + perm_unit(q, j);
      const bool ok = c >= 0 && o < L.out;
      const float val = pg[ok ? L.w_off + o * L.ld + c : L.w_off];
      P::set(fr, j, ok ? val : 0.f);
    }
    w0t[f] = fr;
  }
}

// bit 16 b + 4 u + r: pre-activation of unit 16u + 4q + r, row block b, is > 0
DLAP_DEV uint32_t sign_bits(const f32x4 (&a)[2][4]) {
  uint32_t m = 0;
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) m |= (a[b][u][r] > 0.f ? 1u : 0u) << (16 * b + 4 * u + r);
  return m;
}
// d gated by the sign word, packed into the k-permuted operand fragments
template <class P>
DLAP_DEV void gate_bits(const f32x4 (&d)[2][4], uint32_t m, typename P::Frag (&out)[2][2]) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f32x4 lo = d[b][2 * s], hi = d[b][2 * s + 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        lo[r] = ((m >> (16 * b + 8 * s + r)) & 1u) ? lo[r] : 0.f;
        hi[r] = ((m >> (16 * b + 8 * s + 4 + r)) & 1u) ? hi[r] : 0.f;
      }
      out[b][s] = P::pack(lo, hi);
    }
}

// One tile: dx[b][v] = lane (q, n): d w / d (panel column 16v + 4q + r) of row n of block b,
// scaled by sc[b] (0 for a row beyond R).
template <class P, int KS1, int NL>
DLAP_DEV void sens_tile(const MlpDims& D, const typename P::Frag* lds, const float* aux,
                        const typename P::Frag* w0t, const typename P::Frag (&xf)[2][KS1], const float (&sc)[2],
                        f32x4 (&dx)[2][2 * KS1]) {
  using Frag = typename P::Frag;
  const int q = lane_id() >> 4;
  f32x4 a[2][4];
  Frag pf[2][2];
  uint32_t sg[NL];
  {
    f32x4 init[2][4];
    bias_init<4>(aux + D.a_sb, init);
    layer0<P, KS1, 4>(lds, D.s_fwd0, xf, init, a);
  }
  sg[0] = sign_bits(a);
#pragma unroll
  for (int j = 1; j < NL; ++j) {
    act_tile<P, 4, false>(a, 0xFFFFFFFFu, pf);
    layer_chain<P, 4, 2>(lds, D.s_fwd + (j - 1) * 8, pf, a, aux + D.a_sb + 64 * j);
    sg[j] = sign_bits(a);
  }
  Frag dzf[2][2];
  {
    f32x4 t[2][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const f32x4 ww = ld4(aux + D.a_wo + 16 * u + 4 * q);
      t[0][u] = sc[0] * ww;
      t[1][u] = sc[1] * ww;
    }
    gate_bits<P>(t, sg[NL - 1], dzf);
  }
#pragma unroll
  for (int j = NL - 1; j > 0; --j) {
    f32x4 da[2][4];
    layer_chain<P, 4, 2>(lds, D.s_bwd + (j - 1) * 8, dzf, da);
    gate_bits<P>(da, sg[j - 1], dzf);
  }
#pragma unroll
  for (int v = 0; v < 2 * KS1; ++v) {
    f32x4 c0 = zero4(), c1 = zero4();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const Frag w = ldsf(w0t, 2 * v + s);
      c0 = P::mma(w, dzf[0][s], c0);
      c1 = P::mma(w, dzf[1][s], c1);
    }
    dx[0][v] = c0; dx[1][v] = c1;
  }
}

DLAP_DEV f32x4 abs4(const f32x4& v) { return __builtin_elementwise_abs(v); }
