// Variable importance: the gradient of the raw SDF weight with respect to the whole layer-0 input
// row (the F characteristics and the Dm per-period columns), reduced over the compacted rows of a
// split. An analysis pass beside the training kernels: nothing here runs inside an epoch graph.
//
// Reference op: torch autograd of `SDFNetwork.forward` in evaluation mode (Linear -> ReLU per
// hidden layer, output_proj) with respect to its concatenated input, d w_raw / d [x ; state].
//
// Per 32-row tile (T orientation of k_mlp.hip: a block is 16 units x 16 rows, lane (q, n) holds
// unit 16u + 4q + r of row n):
//   forward   evaluation weights, no dropout; of every hidden layer only the ReLU sign is kept
//             (one bit per unit and row: a 32-bit word per layer and lane);
//   backward  dz_L = s[g][t] * w_out gated by sign(z_L) (|s| in the chain, the sign of s applied to
//             the result), then dz_{j-1} = (W_j^T . dz_j) gated, through the transposed chain
//             fragments (s_bwd) down to dz_0 [64 x 32];
//   input     dx^T = W0^T . dz_0 -- W0^T [KP x 64] as A operand with the hidden unit on the
//             (permuted) k axis. That fragment set is not in the blob: the prologue of every model
//             builds it in LDS from the model's fp32 parameters (panel column k < F -> W0 column k,
//             [ppc, ppc + Dm) -> W0 column F + k - ppc, zero elsewhere).
// (The per-tile pieces live in sens_dev.h: k_macro_sens.hip runs the same chain.)
// Reductions over the valid rows, per panel column: abs[g] = sum |dx_g|, sum[g] = sum dx_g and
// ens = sum | sum_g dx_g | (dx_g carries the scale, so this is the ensemble weight's gradient).
//
// Model-outer: a workgroup owns a chunk of 4 * kTPW consecutive tiles (wave w: tiles
// 4 k + w of the chunk). For each model it stages that model's SDF fragments and walks the chunk;
// the signed tile gradients add up in registers that live across the model loop, and |.| is taken
// after the last model -- no [G][R][C] intermediate. Determinism: no atomics; a lane sums its
// tiles in order, the 16 row lanes combine by a fixed shuffle tree, the four waves as
// (w0 + w1) + (w2 + w3) through LDS, and one partial per chunk goes to HBM; k_sens_reduce sums the
// chunks in index order in fp64. The chunk partition depends on R only and a model's partial on
// nothing but its own weights and scale, so abs / sum of a member have the same bits alone,
// batched, and at any position of the batch.
// Rows beyond R get scale 0 and a zero panel row (their clamped loads stay inside the arrays);
// per-period inputs and scales are read only for the periods of the rows present.
#include <algorithm>
#include "common.h"
#include "layout.h"
#include "mlp.h"
#include "tower_dev.h"
#include "sens_dev.h"

namespace {

constexpr int kTPW = 2;              // tiles per wave and chunk
constexpr int kChunkTiles = 4 * kTPW;

__host__ __device__ inline size_t sens_lds_bytes(const MlpDims& D, int KS1) {
  return sens_red_base(D, KS1) + (size_t)4 * 2 * 32 * KS1 * sizeof(float);
}

// Sum over the 16 row lanes (fixed shuffle tree), then over the four waves as (w0 + w1) + (w2 + w3);
// row `row` of the chunk's partial block ([2 G + 1][KP] floats) gets the KP column sums.
template <int KS1>
DLAP_DEV void sens_combine(const f32x4 (&acc)[2 * KS1], float* red, float* dst) {
  constexpr int KP = 32 * KS1;
  const int lane = lane_id(), wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  __syncthreads();                                     // the previous combine's reads are done
#pragma unroll
  for (int v = 0; v < 2 * KS1; ++v)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = acc[v][r];
      x += __shfl_xor(x, 1, 64); x += __shfl_xor(x, 2, 64);
      x += __shfl_xor(x, 4, 64); x += __shfl_xor(x, 8, 64);
      if (n == 0) red[wave * KP + 16 * v + 4 * q + r] = x;
    }
  __syncthreads();
  for (int c = threadIdx.x; c < KP; c += blockDim.x)
    *gp(dst + c) = (red[c] + red[KP + c]) + (red[2 * KP + c] + red[3 * KP + c]);
}

template <class P, int KS1, int NL>
__global__ __launch_bounds__(256, 1) void k_input_sens(const MlpJob* __restrict__ jobs, const SensJob* __restrict__ sj,
                                                       MlpDims D, PackLayer L0, int G, float* __restrict__ part) {
  using Frag = typename P::Frag;
  constexpr int KP = 32 * KS1, VB = 2 * KS1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Frag* lds = reinterpret_cast<Frag*>(smem);
  float* aux = aux_lds_ptr(smem, D);
  float* spp = pp_lds_ptr(smem, D);
  Frag* w0t = reinterpret_cast<Frag*>(smem + sens_w0t_base(D));
  float* red = reinterpret_cast<float*>(smem + sens_red_base(D, KS1));
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int tile0 = blockIdx.x * kChunkTiles + wave;          // this wave's tiles: tile0 + 4 k
  float* pblk = part + (size_t)blockIdx.x * (2 * G + 1) * KP;
  f32x4 ens[kTPW][2][VB];
#pragma unroll
  for (int k = 0; k < kTPW; ++k)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < VB; ++v) ens[k][b][v] = zero4();
  for (int g = 0; g < G; ++g) {
    const MlpJob J = jobs[g];
    const SensJob S = sj[g];
    DLAP_ASSERT(J.R > 0);
    TileIn<P, KS1> in[kTPW];
#pragma unroll
    for (int k = 0; k < kTPW; ++k) issue_tile<P, KS1, false>(J, tile0 + 4 * k, in[k]);   // rows clamped to R - 1
    __syncthreads();                                   // every wave is done with the previous model's image
    build_w0t<P, KS1>(w0t, S.params, L0, D);
    stage_weights<P>(J, D, lds, aux, spp);             // (ends with a barrier: w0t is complete too)
    f32x4 ab[VB], sm[VB];
#pragma unroll
    for (int v = 0; v < VB; ++v) ab[v] = sm[v] = zero4();
#pragma unroll
    for (int k = 0; k < kTPW; ++k) {
      const int oz = opaque_zero();                    // no weight fragment kept across tiles
      const int tile = tile0 + 4 * k;
      Frag xf[2][KS1];
      const RowInfo ri = finish_tile<P, KS1>(J, D, tile, in[k], xf, spp);
      // the chain is seeded with |s| and the sign of s goes onto the finished gradient: the bf16
      // MFMA's internal sum is not sign-symmetric, and this way scales s and -s of one model give
      // gradients that cancel exactly
      float sc[2], sgn[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        DLAP_ASSERT((unsigned)ri.t[b] < (unsigned)J.T);
        const float s = *gp32(S.scale, (uint32_t)ri.t[b]);
        sc[b] = ri.dense[b] >= 0 ? fabsf(s) : 0.f;
        sgn[b] = s < 0.f ? -1.f : 1.f;
      }
      f32x4 dx[2][VB];
      sens_tile<P, KS1, NL>(D, lds + oz, aux + oz, w0t + oz, xf, sc, dx);
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int v = 0; v < VB; ++v) {
          dx[b][v] *= sgn[b];
          ab[v] += abs4(dx[b][v]);
          sm[v] += dx[b][v];
          ens[k][b][v] += dx[b][v];
        }
    }
    sens_combine<KS1>(ab, red, pblk + (size_t)(2 * g) * KP);
    sens_combine<KS1>(sm, red, pblk + (size_t)(2 * g + 1) * KP);
  }
  // |.| of the summed members, rows in the order of the per-model sums (so one model with scale 1
  // gives ens == abs bit for bit)
  f32x4 ea[VB];
#pragma unroll
  for (int v = 0; v < VB; ++v) ea[v] = zero4();
#pragma unroll
  for (int k = 0; k < kTPW; ++k)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < VB; ++v) ea[v] += abs4(ens[k][b][v]);
  sens_combine<KS1>(ea, red, pblk + (size_t)(2 * G) * KP);
  (void)lane;
}

// out[row][c] (fp64, row < 2 G + 1, c < C = F + Dm) = the chunk partials summed in index order;
// input column c sits in panel column c (c < F) or ppc + c - F.
__global__ __launch_bounds__(256) void k_sens_reduce(const float* __restrict__ part, int nchunks, int nrows, int KP,
                                                    int F, int C, int ppc, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows * C) return;
  const int row = i / C, c = i - row * C;
  const int k = c < F ? c : ppc + (c - F);
  const auto src = gp(part) + (size_t)row * KP + k;
  const size_t stride = (size_t)nrows * KP;
  double acc = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) acc += (double)src[ch * stride];
  *gp(out + i) = acc;
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
// Shapes covered: the fused layer-0 path (panel row of 64 or 128 columns), 1..4 hidden layers of
// <= 64 units, bf16 and fp32, as long as the LDS image (SDF fragments, aux, staged per-period
// inputs, W0^T) fits 160 KiB -- fp32 towers with four layers on a 128-column row do not.
bool sens_supported(const MlpDims& D0, int KS1) {
  if (D0.wide || (KS1 != 2 && KS1 != 4)) return false;
  if (D0.nl_sdf < 1 || D0.nl_sdf > 4) return false;
  if (D0.F + D0.Dm > 32 * KS1 || D0.ppc < D0.F || D0.ppc + D0.Dm > 32 * KS1) return false;
  return sens_lds_bytes(sens_dims(D0), KS1) <= 160 * 1024;
}

int sens_chunks(int R) { return (((R + 31) >> 5) + kChunkTiles - 1) / kChunkTiles; }
size_t sens_part_floats(int R, int G, int KS1) { return (size_t)sens_chunks(R) * (2 * G + 1) * 32 * KS1; }

void launch_input_sens(const MlpJob* jobs, const SensJob* sj, int G, int R, const MlpDims& D0, int KS1,
                       const PackLayer& L0, float* part, double* out, hipStream_t st) {
  if (!sens_supported(D0, KS1) || R <= 0 || G <= 0)
    dlap_throw_hip(hipErrorInvalidValue, "input_sens: unsupported shape", __FILE__, __LINE__);
  const MlpDims D = sens_dims(D0);
  const size_t sh = sens_lds_bytes(D, KS1);
  const int nch = sens_chunks(R);
  dim3 grid(nch), block(256);
#define SENS_NL(PP, KS, N) if (D.nl_sdf == N) \
    hipLaunchKernelGGL((k_input_sens<PP, KS, N>), grid, block, sh, st, jobs, sj, D, L0, G, part);
#define SENS_KS(PP, KS) if (KS1 == KS) { SENS_NL(PP, KS, 1) SENS_NL(PP, KS, 2) SENS_NL(PP, KS, 3) SENS_NL(PP, KS, 4) }
  if (D.fp32) { SENS_KS(PrecF32, 2) SENS_KS(PrecF32, 4) }
  else { SENS_KS(PrecBF16, 2) SENS_KS(PrecBF16, 4) }
#undef SENS_KS
#undef SENS_NL
  HIP_OK(hipGetLastError());
  const int C = D.F + D.Dm, nrows = 2 * G + 1;
  hipLaunchKernelGGL(k_sens_reduce, dim3((nrows * C + 255) / 256), dim3(256), 0, st, part, nch, nrows, 32 * KS1,
                     D.F, C, D.ppc, out);
  HIP_OK(hipGetLastError());
}
