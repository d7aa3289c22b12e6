// Macro importance through the LSTM: the gradient of the (scaled) raw SDF weight of a row (t, i)
// with respect to the standardised macro series fed at period t - l, reduced over the compacted
// rows of a split, for the lags l = 0 .. L - 1 and for their sum. An analysis pass beside
// k_sens.hip; nothing here runs inside an epoch graph.
//
// Reference op: torch autograd of `SDFNetwork.forward` in evaluation mode with respect to the
// `macro` input fed through `macro_lstm` (single layer).
//
// The dependence of a row on the macro history factors through the H state columns:
//   d w_g(t,i) / d m[t-l][j] = sum_k d_g(t,i)[k] * (C_g[t][l] . W_ih,g)[k][j]
//   d_g(t,i)   the row's gradient with respect to the state columns: the [ppc, ppc + H) columns of
//              sens_tile's dx (sens_dev.h), scaled and signed;
//   C_g[t][l]  [H x 4H], the truncated BPTT of the H unit seeds e_k from step t back to step t - l,
//              read at the gate pre-activations -- per period only, produced by k_lstm_lagjac from
//              the saved evaluation recurrence. All of the LSTM side is fp32 in both precisions.
//
// k_lstm_lagjac: one wave per (model, period), lane (k, j) = seed k, unit j. Per lag
//   dc = lc + lh o (1 - tanh(c)^2);  dpre = (dc g i(1-i), dc c_prev f(1-f), dc i (1-g^2), lh tanh(c) o(1-o))
//   C[t][l][k] = dpre;  lh <- W_hh^T dpre (through LDS, fixed order);  lc <- dc f
// with c_prev = c0 at step 0 and zeros where t - l < 0. Slot l = L holds the sum over the lags.
//
// k_macro_sens: a workgroup owns a chunk of kRounds rounds of 8 tiles (wave w: tiles 4 k + w of the
// round). Per round
//   1. model-outer, as k_input_sens: stage the model's SDF fragments, run sens_tile on the wave's
//      two tiles, broadcast the H state-column gradients of every row to the four lane groups
//      (the row sits on the MFMA n axis) and keep them in registers and, for step 2, in LDS. Then
//      per lag and group of four 16-series blocks: u[row] = d[row] . C_g[t(row)][l] on the VALU
//      (the period is per lane: a block may span periods), prod = W_ih,g^T . u on
//      v_mfma_f32_16x16x4_f32 (k index (q, s) = gate row q H + s; the W_ih^T elements are read
//      through L2, 16 consecutive series per lane group), and sum_rows |prod| -> abs[g][l].
//   2. after the last model, per lag (and the lag sum) and block group: the members' products are
//      chained in one accumulator (a GEMM with K = G 4H), then sum_rows |.| -> ens[l]. The
//      products are formed a second time here: keeping every lag's signed 32 x M tile of a wave
//      across the model loop would take (L + 1) x 96 VGPRs.
// Determinism: no atomics. A lane sums its tiles in order, the 16 row lanes combine by a fixed
// shuffle tree, the four waves as (w0 + w1) + (w2 + w3) through LDS, the rounds of a chunk add up
// in order in the chunk's partial, and k_macro_reduce sums the chunks in index order in fp64. The
// partition depends on R only and a member's abs on nothing but its own weights and scale: same
// bits alone, batched, and at any batch position. With one model of scale one the ens accumulator
// sees exactly the abs pass's MFMA chain, so ens == abs bit for bit.
// Rows beyond R carry scale 0 (their clamped period index stays inside C).
#include <algorithm>
#include "common.h"
#include "layout.h"
#include "mlp.h"
#include "tower_dev.h"
#include "sens_dev.h"
#include "macro_sens.h"

namespace {

constexpr int kTPW = 2;                      // tiles per wave and round
constexpr int kRoundTiles = 4 * kTPW;
constexpr int kRounds = 4;                   // rounds per chunk
constexpr int kChunkTiles = kRounds * kRoundTiles;

// LDS: the k_input_sens image up to the W0^T fragments, then the wave-combine scratch (4 x 64
// floats), then the state-column gradients of the round [G][8 tiles][32 rows][HM].
__host__ __device__ inline size_t macro_dst_base(const MlpDims& D, int KS1) { return sens_red_base(D, KS1) + 1024; }
__host__ __device__ inline size_t macro_lds_bytes(const MlpDims& D, int KS1, int G, int HM) {
  return macro_dst_base(D, KS1) + (size_t)G * kRoundTiles * 32 * HM * sizeof(float);
}

template <int HM>
__global__ __launch_bounds__(64) void k_lstm_lagjac(const LagJob* __restrict__ jobs, MacroDims A, float* __restrict__ C) {
  __shared__ float sd[HM * 4 * HM];
  const int t = blockIdx.x, g = blockIdx.y, H = A.H, T = A.T, L = A.L;
  const LagJob J = jobs[g];
  const int lane = threadIdx.x, k = lane / HM, j = lane % HM;
  const bool on = lane < HM * HM && k < H && j < H;
  const int kk = on ? k : 0, jj = on ? j : 0;
  for (int i = lane; i < HM * 4 * HM; i += 64) sd[i] = 0.f;
  // column jj of W_hh: lh[jj] = sum_{q, i} W_hh[q H + i][jj] dpre[q][i]
  float w[4][HM];
  const auto Whh = gp(J.params) + A.w_hh;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < HM; ++i) {
      const bool ok = on && i < H;
      const float v = Whh[ok ? (q * H + i) * H + jj : 0];
      w[q][i] = ok ? v : 0.f;
    }
  const auto sg = gp(J.sg), sc = gp(J.sc);
  constexpr int CS = HM * 4 * HM;
  const auto out = gp(C) + ((size_t)(g * T + t) * (L + 1)) * CS + kk * 4 * HM + jj;
  float lh = on && j == k ? 1.f : 0.f, lc = 0.f;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const int tau = t - l;                            // (uniform)
    if (tau < 0) {
      if (on)
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(size_t)l * CS + q * HM] = 0.f;
      continue;
    }
    const float gi = sg[tau * 4 * H + jj], gf = sg[tau * 4 * H + H + jj];
    const float gg = sg[tau * 4 * H + 2 * H + jj], go = sg[tau * 4 * H + 3 * H + jj];
    const float c = sc[tau * H + jj];
    const float cp = tau > 0 ? sc[(tau - 1) * H + jj] : (J.c0 ? gp(J.c0)[jj] : 0.f);
    const float th = tanhf(c);
    const float dc = lc + lh * go * (1.f - th * th);
    float dp[4];
    dp[0] = dc * gg * gi * (1.f - gi);
    dp[1] = dc * cp * gf * (1.f - gf);
    dp[2] = dc * gi * (1.f - gg * gg);
    dp[3] = lh * th * go * (1.f - go);
    if (on) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        out[(size_t)l * CS + q * HM] = dp[q];
        cs[q] += dp[q];
        sd[(kk * 4 + q) * HM + jj] = dp[q];
      }
    }
    __syncthreads();
    float nh = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < HM; ++i) nh = fmaf(w[q][i], sd[(kk * 4 + q) * HM + i], nh);
    lh = on ? nh : 0.f;
    lc = on ? dc * gf : 0.f;
    __syncthreads();
  }
  if (on)
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(size_t)L * CS + q * HM] = cs[q];
}

// u[s] = sum_k d[k] C[k][q][s]: c points at C[t][l][0][q][0] of the lane's period and lane group
template <int HM>
DLAP_DEV void lag_u(const float (&d)[HM], const DLAP_GLOBAL float* c, float (&u)[HM]) {
#pragma unroll
  for (int s = 0; s < HM; ++s) u[s] = 0.f;
#pragma unroll
  for (int k = 0; k < HM; ++k)
#pragma unroll
    for (int h = 0; h < HM / 4; ++h) {
      const f32x4 cv = ld4(c + k * 4 * HM + 4 * h);
#pragma unroll
      for (int r = 0; r < 4; ++r) u[4 * h + r] = fmaf(d[k], cv[r], u[4 * h + r]);
    }
}

// A operand of k-step s for the 16 series [col - n, col - n + 16): W_ih[q H + s][col] (0 beyond M / H)
template <int HM>
DLAP_DEV void load_wih(const DLAP_GLOBAL float* wih, int H, int M, int col, int q, float (&a)[HM]) {
#pragma unroll
  for (int s = 0; s < HM; ++s) {
    const bool ok = s < H && col < M;
    const float v = wih[ok ? (q * H + s) * M + col : 0];
    a[s] = ok ? v : 0.f;
  }
}

template <int HM>
DLAP_DEV f32x4 mma_u(const float (&a)[HM], const float (&u)[HM], f32x4 c) {
#pragma unroll
  for (int s = 0; s < HM; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], u[s], c, 0, 0, 0);
  return c;
}

// Sum over the 16 row lanes (fixed shuffle tree), then over the four waves as (w0 + w1) + (w2 + w3);
// the 64 column sums are stored to dst (first round of the chunk) or added to it.
DLAP_DEV void macro_combine(const f32x4 (&acc)[4], float* red, float* dst, bool first) {
  const int lane = lane_id(), wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  __syncthreads();                                     // the previous combine's reads are done
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = acc[v][r];
      x += __shfl_xor(x, 1, 64); x += __shfl_xor(x, 2, 64);
      x += __shfl_xor(x, 4, 64); x += __shfl_xor(x, 8, 64);
      if (n == 0) red[wave * 64 + 16 * v + 4 * q + r] = x;
    }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int c = threadIdx.x;
    const float s = (red[c] + red[64 + c]) + (red[128 + c] + red[192 + c]);
    const auto p = gp(dst + c);
    *p = first ? s : *p + s;
  }
}

template <class P, int KS1, int NL, int HM>
__global__ __launch_bounds__(256, 1) void k_macro_sens(const MlpJob* __restrict__ jobs, const SensJob* __restrict__ sj,
                                                       MacroDims A, MlpDims D, PackLayer L0,
                                                       const float* __restrict__ Cb, float* __restrict__ part) {
  using Frag = typename P::Frag;
  constexpr int VB = 2 * KS1, CS = HM * 4 * HM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Frag* lds = reinterpret_cast<Frag*>(smem);
  float* aux = aux_lds_ptr(smem, D);
  float* spp = pp_lds_ptr(smem, D);
  Frag* w0t = reinterpret_cast<Frag*>(smem + sens_w0t_base(D));
  float* red = reinterpret_cast<float*>(smem + sens_red_base(D, KS1));
  float* dst = reinterpret_cast<float*>(smem + macro_dst_base(D, KS1));
  const int lane = lane_id(), wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  const int G = A.G, L = A.L, H = A.H, M = A.M, T = A.T;
  const int nvg = (M + 63) >> 6, MPAD = 64 * nvg;
  const int ntiles = (A.R + 31) >> 5;
  const int ctile0 = blockIdx.x * kChunkTiles;
  const int nrounds = min(kRounds, (ntiles - ctile0 + kRoundTiles - 1) / kRoundTiles);
  float* pblk = part + (size_t)blockIdx.x * (G * L + L + 1) * MPAD;
  const auto Cg = gp(Cb);
  for (int round = 0; round < nrounds; ++round) {
    const int tile0 = ctile0 + round * kRoundTiles + wave;      // this wave's tiles: tile0 + 4 k
    const bool first = round == 0;
    int tp[kTPW][2];                                            // period of the lane's row
    for (int g = 0; g < G; ++g) {
      const MlpJob J = jobs[g];
      const SensJob S = sj[g];
      DLAP_ASSERT(J.R > 0);
      TileIn<P, KS1> in[kTPW];
#pragma unroll
      for (int k = 0; k < kTPW; ++k) issue_tile<P, KS1, false>(J, tile0 + 4 * k, in[k]);   // rows clamped to R - 1
      __syncthreads();                                 // every wave is done with the previous model's image
      build_w0t<P, KS1>(w0t, S.params, L0, D);
      stage_weights<P>(J, D, lds, aux, spp);           // (ends with a barrier: w0t is complete too)
      float d[kTPW][2][HM];
#pragma unroll
      for (int k = 0; k < kTPW; ++k) {
        const int oz = opaque_zero();                  // no weight fragment kept across tiles
        const int tile = tile0 + 4 * k;
        Frag xf[2][KS1];
        const RowInfo ri = finish_tile<P, KS1>(J, D, tile, in[k], xf, spp);
        float sc[2], sgn[2];                           // |s| in the chain, the sign on the result (k_sens.hip)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          DLAP_ASSERT((unsigned)ri.t[b] < (unsigned)J.T);
          const float s = *gp32(S.scale, (uint32_t)ri.t[b]);
          sc[b] = ri.dense[b] >= 0 ? fabsf(s) : 0.f;
          sgn[b] = s < 0.f ? -1.f : 1.f;
          tp[k][b] = ri.t[b];
        }
        f32x4 dx[2][VB];
        sens_tile<P, KS1, NL>(D, lds + oz, aux + oz, w0t + oz, xf, sc, dx);
        // the state columns are the panel row's last eight: column ppc + kk sits in block VB - 1 on
        // lane group 2 + kk / 4, element kk % 4 (columns >= H carry zero W0^T, so d = 0 there)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          float* row = dst + ((size_t)(g * kRoundTiles + wave * kTPW + k) * 32 + 16 * b + n) * HM;
#pragma unroll
          for (int kk = 0; kk < HM; ++kk) {
            const float x = dx[b][VB - 1][kk & 3] * sgn[b];
            d[k][b][kk] = __shfl(x, 32 + 16 * (kk >> 2) + n, 64);
            if (q == 0) row[kk] = d[k][b][kk];
          }
        }
      }
      const auto wih = gp(S.params) + A.w_ih;
      for (int l = 0; l < L; ++l)
        for (int vg = 0; vg < nvg; ++vg) {
          float a[4][HM];
#pragma unroll
          for (int v = 0; v < 4; ++v) load_wih<HM>(wih, H, M, 64 * vg + 16 * v + n, q, a[v]);
          f32x4 acc[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[v] = zero4();
#pragma unroll
          for (int k = 0; k < kTPW; ++k)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              DLAP_ASSERT((unsigned)tp[k][b] < (unsigned)T);
              float u[HM];
              lag_u<HM>(d[k][b], Cg + ((size_t)(g * T + tp[k][b]) * (L + 1) + l) * CS + q * HM, u);
#pragma unroll
              for (int v = 0; v < 4; ++v) acc[v] += abs4(mma_u<HM>(a[v], u, zero4()));
            }
          macro_combine(acc, red, pblk + (size_t)(g * L + l) * MPAD + 64 * vg, first);
        }
    }
    __syncthreads();                                   // the round's state gradients are in LDS
    // |.| of the summed members, tiles and blocks in the order of the per-model sums
    for (int l = 0; l <= L; ++l)
      for (int vg = 0; vg < nvg; ++vg) {
        f32x4 acc[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] = zero4();
#pragma unroll
        for (int k = 0; k < kTPW; ++k) {
          f32x4 e[2][4];
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) e[b][v] = zero4();
          for (int g = 0; g < G; ++g) {
            const auto wih = gp(sj[g].params) + A.w_ih;
            float a[4][HM];
#pragma unroll
            for (int v = 0; v < 4; ++v) load_wih<HM>(wih, H, M, 64 * vg + 16 * v + n, q, a[v]);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const float* row = dst + ((size_t)(g * kRoundTiles + wave * kTPW + k) * 32 + 16 * b + n) * HM;
              float dd[HM], u[HM];
#pragma unroll
              for (int kk = 0; kk < HM; ++kk) dd[kk] = row[kk];
              lag_u<HM>(dd, Cg + ((size_t)(g * T + tp[k][b]) * (L + 1) + l) * CS + q * HM, u);
#pragma unroll
              for (int v = 0; v < 4; ++v) e[b][v] = mma_u<HM>(a[v], u, e[b][v]);
            }
          }
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] += abs4(e[b][v]);
        }
        macro_combine(acc, red, pblk + (size_t)(G * L + l) * MPAD + 64 * vg, first);
      }
  }
  (void)lane;
}

// out[row][j] (fp64, j < M) = the chunk partials summed in index order
__global__ __launch_bounds__(256) void k_macro_reduce(const float* __restrict__ part, int nchunks, int nrows, int MPAD,
                                                     int M, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows * M) return;
  const int row = i / M, j = i - row * M;
  const auto src = gp(part) + (size_t)row * MPAD + j;
  const size_t stride = (size_t)nrows * MPAD;
  double acc = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) acc += (double)src[ch * stride];
  *gp(out + i) = acc;
}

int macro_mpad(int M) { return ((M + 63) >> 6) * 64; }

}  // namespace

// ---- host side ------------------------------------------------------------------------------
bool macro_sens_supported(const MlpDims& D0, int KS1, int nrnn, int H, int G) {
  if (!sens_supported(D0, KS1)) return false;
  if (nrnn != 1 || H < 1 || H > 8 || D0.Dm != H || G < 1) return false;
  if (D0.ppc != 32 * KS1 - 8) return false;          // the state columns are the row's last eight
  return macro_lds_bytes(sens_dims(D0), KS1, G, macro_hm(H)) <= 160 * 1024;
}

int macro_chunks(int R) { return (((R + 31) >> 5) + kChunkTiles - 1) / kChunkTiles; }
size_t macro_c_floats(const MacroDims& A) {
  const int HM = macro_hm(A.H);
  return (size_t)A.G * A.T * (A.L + 1) * HM * 4 * HM;
}
size_t macro_part_floats(const MacroDims& A) {
  return (size_t)macro_chunks(A.R) * (A.G * A.L + A.L + 1) * macro_mpad(A.M);
}
size_t macro_out_doubles(const MacroDims& A) { return (size_t)(A.G * A.L + A.L + 1) * A.M; }

void launch_lstm_lagjac(const LagJob* jobs, const MacroDims& A, float* C, hipStream_t st) {
  if (A.G <= 0 || A.T <= 0 || A.L < 1 || A.L > A.T || A.H < 1 || A.H > 8)
    dlap_throw_hip(hipErrorInvalidValue, "lstm_lagjac: unsupported shape", __FILE__, __LINE__);
  dim3 grid(A.T, A.G), block(64);
  if (macro_hm(A.H) == 4) hipLaunchKernelGGL((k_lstm_lagjac<4>), grid, block, 0, st, jobs, A, C);
  else hipLaunchKernelGGL((k_lstm_lagjac<8>), grid, block, 0, st, jobs, A, C);
  HIP_OK(hipGetLastError());
}

void launch_macro_sens(const MlpJob* jobs, const SensJob* sj, const MacroDims& A, const MlpDims& D0, int KS1,
                       const PackLayer& L0, const float* C, float* part, double* out, hipStream_t st) {
  if (!macro_sens_supported(D0, KS1, 1, A.H, A.G) || A.R <= 0 || A.M <= 0 || A.L < 1 || A.L > A.T)
    dlap_throw_hip(hipErrorInvalidValue, "macro_sens: unsupported shape", __FILE__, __LINE__);
  const MlpDims D = sens_dims(D0);
  const int HM = macro_hm(A.H);
  const size_t sh = macro_lds_bytes(D, KS1, A.G, HM);
  const int nch = macro_chunks(A.R);
  dim3 grid(nch), block(256);
#define MS_NL(PP, KS, HH, N) if (D.nl_sdf == N) \
    hipLaunchKernelGGL((k_macro_sens<PP, KS, N, HH>), grid, block, sh, st, jobs, sj, A, D, L0, C, part);
#define MS_H(PP, KS, HH) if (HM == HH) { MS_NL(PP, KS, HH, 1) MS_NL(PP, KS, HH, 2) MS_NL(PP, KS, HH, 3) MS_NL(PP, KS, HH, 4) }
#define MS_KS(PP, KS) if (KS1 == KS) { MS_H(PP, KS, 4) MS_H(PP, KS, 8) }
  if (D.fp32) { MS_KS(PrecF32, 2) MS_KS(PrecF32, 4) }
  else { MS_KS(PrecBF16, 2) MS_KS(PrecBF16, 4) }
#undef MS_KS
#undef MS_H
#undef MS_NL
  HIP_OK(hipGetLastError());
  const int nrows = A.G * A.L + A.L + 1;
  hipLaunchKernelGGL(k_macro_reduce, dim3((nrows * A.M + 255) / 256), dim3(256), 0, st, part, nch, nrows,
                     macro_mpad(A.M), A.M, out);
  HIP_OK(hipGetLastError());
}
