// Characteristic knock-outs: the ensemble SDF of a split under many scenarios, each a set of
// characteristic columns replaced by a base row (definition in knock.h). An analysis pass beside
// the training kernels: nothing here runs inside an epoch graph.
//
// Reference op: `SDFNetwork.forward` in evaluation mode on the panel with the scenario's columns
// overwritten, `zero_mean_normalize`, the L1 normalisation and the model average of
// `evaluate_ensemble`, per scenario (analysis/knockout.py).
//
//   k_knock_fwd      model-outer, as k_input_sens: a workgroup owns 4 * kTPW consecutive 32-row
//                    tiles of the resident panel (wave w: tiles 4 k + w of the chunk). For each
//                    model it stages the evaluation blob, aux and the split's per-period inputs; a
//                    wave loads a tile once (issue_tile / finish_tile, so the per-period columns are
//                    inserted as in the forward) and, per scenario, replaces the fragment elements
//                    whose column bit is set in the scenario's mask by the base row's -- built once
//                    per wave with the conversion the panel upload uses (P::set) -- and runs the
//                    forward's own layer0 / sdf_forward_tile. Layer 0 is recomputed per scenario,
//                    so a raw weight has the bits forward_split gives on a panel uploaded with
//                    those columns replaced. The 32 raw weights go to wk[k][g][row]; no atomics,
//                    one lane stores each element once; rows beyond R are clamped loads and are
//                    not stored.
//   k_knock_reduce   one workgroup per (period, scenario) walks the period's rows in three stages:
//                    per member S1, then SA and SR (from which c_g and s_g), then e with EA, E2,
//                    ER (and sum_r, sum_rr), then the optional dense write. Sums: fp64 per lane
//                    over rows tid, tid + 256, .., a fixed xor-shuffle tree over the 64 lanes, the
//                    four waves in order through LDS. A sum depends on wk[k] of its own scenario
//                    (and member) and the panel only: not on the chunking, the scenario's position
//                    or the other members.
// LDS of k_knock_fwd: [blob | aux | pp [T][ppst]] (tower_dev.h), then the masks of a full chunk.
#include <algorithm>
#include "common.h"
#include "layout.h"
#include "mlp.h"
#include "tower_dev.h"
#include "knock.h"

namespace {

constexpr int kTPW = 4;              // tiles per wave and workgroup
constexpr int kRT = 256;             // threads of k_knock_reduce
constexpr int kRW = kRT / 64;

// launch dims: the periods' inputs are always staged (T of the split)
MlpDims knock_dims(const MlpDims& D0, int T) {
  MlpDims D = D0;
  D.pp_lds_floats = D0.Dm > 0 ? T * D0.ppst : 0;
  return D;
}
__host__ __device__ inline size_t knock_mask_base(const MlpDims& D) { return (lds_bytes_of(D) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t knock_lds_bytes(const MlpDims& D, int KS1) {
  return knock_mask_base(D) + (size_t)KNOCK_MAX_CHUNK * KS1 * sizeof(uint32_t);
}

template <class P, int KS1>
__global__ __launch_bounds__(256, P::kF32 ? 1 : 2)
void k_knock_fwd(const MlpJob* __restrict__ jobs, KnockArgs A, MlpDims D) {
  using Frag = typename P::Frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Frag* lds = reinterpret_cast<Frag*>(smem);
  float* aux = aux_lds_ptr(smem, D);
  float* spp = pp_lds_ptr(smem, D);
  uint32_t* smask = reinterpret_cast<uint32_t*>(smem + knock_mask_base(D));      // [K][KS1]
  const int lane = lane_id(), wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  const int ntiles = (A.R + 31) >> 5;
  const int tile0 = blockIdx.x * (4 * kTPW) + wave;           // this wave's tiles: tile0 + 4 k
  for (int i = threadIdx.x; i < A.K * KS1; i += blockDim.x) smask[i] = gp(A.masks)[i];
  // the base row's fragments do not depend on the row
  Frag bf[KS1];
#pragma unroll
  for (int s = 0; s < KS1; ++s) {
    const int c0 = 32 * s + 8 * q;
    const f32x4 lo = ld4(gp(A.base) + c0), hi = ld4(gp(A.base) + c0 + 4);
    bf[s] = P::zero();
#pragma unroll
    for (int j = 0; j < 8; ++j) P::set(bf[s], j, j < 4 ? lo[j & 3] : hi[j & 3]);
  }
  const uint32_t kw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  for (int g = 0; g < A.G; ++g) {
    const MlpJob J = jobs[g];
    DLAP_ASSERT(J.R == A.R && J.T == A.T);
    __syncthreads();                                   // every wave is done with the previous model's image
    stage_weights<P>(J, D, lds, aux, spp);             // (ends with a barrier: the masks are complete too)
#pragma unroll 1
    for (int kt = 0; kt < kTPW; ++kt) {
      const int tile = tile0 + 4 * kt;
      if (tile >= ntiles) break;                       // wave-uniform; no barrier below
      TileIn<P, KS1> in;
      issue_tile<P, KS1, false>(J, tile, in);          // rows clamped to R - 1
      Frag xf[2][KS1];
      finish_tile<P, KS1>(J, D, tile, in, xf, spp);
      float* dst = A.wk + (size_t)g * A.R + tile * 32 + n;
#pragma unroll 1
      for (int k = 0; k < A.K; ++k) {
        const int oz = opaque_zero();                  // no weight fragment kept across scenarios
        const Frag* ldt = lds + oz;
        const float* auxt = aux + oz;
        MlpDims Dt = D;
        Dt.nl_sdf += oz;
        Frag xk[2][KS1];
#pragma unroll
        for (int s = 0; s < KS1; ++s) {
          const uint32_t m = smask[k * KS1 + s] >> (8 * q);
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            xk[b][s] = xf[b][s];
#pragma unroll
            for (int j = 0; j < 8; ++j) xk[b][s][j] = ((m >> j) & 1u) ? bf[s][j] : xf[b][s][j];
          }
        }
        auto l0 = [&](f32x4 (&a)[2][4]) {
          f32x4 init[2][4];
          bias_init<4>(auxt + D.a_sb, init);
          layer0<P, KS1, 4>(ldt, D.s_fwd0, xk, init, a);
        };
        float w[2];
        sdf_forward_tile<P, false>(ldt, auxt, Dt, kw, l0, w);
        if (q == 0) {
          float* d = dst + (size_t)k * A.G * A.R;
          if (tile * 32 + n < A.R) *gp(d) = w[0];
          if (tile * 32 + 16 + n < A.R) *gp(d + 16) = w[1];
        }
      }
    }
  }
}

}  // namespace

// The reductions are the definition's arithmetic as written: no product is fused into a sum.
#pragma clang fp contract(off)

namespace {

DLAP_DEV double lane_tree(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
// v[j] <- the sum of v[j] over the workgroup, on every thread: the 64 lanes by the xor tree, the
// waves in order. red: kRW * NV doubles.
template <int NV>
DLAP_DEV void block_sums(double (&v)[NV], double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();                                     // the previous sums have been read
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const double x = lane_tree(v[j]);
    if (lane == 0) red[w * NV + j] = x;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double s = red[j];
#pragma unroll
    for (int k = 1; k < kRW; ++k) s += red[k * NV + j];
    v[j] = s;
  }
}

__global__ __launch_bounds__(kRT) void k_knock_reduce(KnockReduceArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);                       // [kRW][5]
  float* cs = reinterpret_cast<float*>(smem + (size_t)kRW * 5 * sizeof(double));   // [G] c_g
  float* ss = cs + a.G;                                                // [G] s_g
  const int t = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, T = a.pv.T, G = a.G;
  const int r0 = gp(a.pv.row_ptr)[t], cnt = gp(a.pv.row_ptr)[t + 1] - r0;
  const size_t KT = (size_t)a.K * T, KGT = KT * G;
  const size_t eo = (size_t)k * T + t;
  const auto wk = gp(a.wk) + (size_t)k * G * a.R + r0;
  const auto Rc = gp(a.pv.Rc) + r0;
  for (int g = 0; g < G; ++g) {
    const auto w = wk + (size_t)g * a.R;
    double s1[1] = {0.0};
    for (int i = tid; i < cnt; i += kRT) s1[0] += (double)w[i];
    block_sums<1>(s1, red);
    const float c = a.normalize_w ? (float)(s1[0] / (double)max(cnt, 1)) : 0.f;
    double s2[2] = {0.0, 0.0};
    for (int i = tid; i < cnt; i += kRT) {
      const double v = (double)(w[i] - c);
      s2[0] += fabs(v);
      s2[1] += v * (double)Rc[i];
    }
    block_sums<2>(s2, red);
    const float sc = (float)(1.0 / ((double)G * (double)fmaxf((float)s2[0], 1e-8f)));
    if (tid == 0) {
      const size_t mo = ((size_t)k * G + g) * T + t;
      gp(a.mem)[mo] = s1[0];
      gp(a.mem)[KGT + mo] = s2[0];
      gp(a.mem)[2 * KGT + mo] = s2[1];
      cs[g] = c;
      ss[g] = sc;
    }
  }
  __syncthreads();
  double s3[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < cnt; i += kRT) {
    float e = 0.f;
    for (int g = 0; g < G; ++g) e = __builtin_fmaf(wk[(size_t)g * a.R + i] - cs[g], ss[g], e);
    const double ed = (double)e, Rd = (double)Rc[i];
    s3[0] += fabs(ed);
    s3[1] += ed * ed;
    s3[2] += ed * Rd;
    s3[3] += Rd;
    s3[4] += Rd * Rd;
  }
  block_sums<5>(s3, red);
  if (tid == 0) {
    gp(a.ens)[eo] = s3[0];
    gp(a.ens)[KT + eo] = s3[1];
    gp(a.ens)[2 * KT + eo] = s3[2];
    if (a.per && k == 0) {
      gp(a.per)[t] = (double)cnt;
      gp(a.per)[T + t] = s3[3];
      gp(a.per)[2 * T + t] = s3[4];
    }
  }
  if (a.dense) {
    const double ea = s3[0];
    const auto ti = gp(a.pv.rowti) + r0;
    const auto out = gp(a.dense) + eo * a.pv.N;
    for (int i = tid; i < cnt; i += kRT) {
      float e = 0.f;
      for (int g = 0; g < G; ++g) e = __builtin_fmaf(wk[(size_t)g * a.R + i] - cs[g], ss[g], e);
      out[ti[i].y] = ea > 1e-8 ? (float)((double)e / ea) : e;
    }
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
bool knock_supported(const MlpDims& D0, int KS1, int T) {
  if (D0.wide || (KS1 != 2 && KS1 != 4) || T < 1 || T > 65535) return false;
  if (D0.nl_sdf < 1 || D0.nl_sdf > 4) return false;
  if (D0.F + D0.Dm > 32 * KS1 || D0.ppc < D0.F || D0.ppc + D0.Dm > 32 * KS1) return false;
  return knock_lds_bytes(knock_dims(D0, T), KS1) <= 160 * 1024;
}

void launch_knock_fwd(const MlpJob* jobs, const KnockArgs& A, const MlpDims& D0, int KS1, hipStream_t st) {
  if (!knock_supported(D0, KS1, A.T) || A.R <= 0 || A.G <= 0 || A.K < 1 || A.K > KNOCK_MAX_CHUNK)
    dlap_throw_hip(hipErrorInvalidValue, "knockout: unsupported shape", __FILE__, __LINE__);
  const MlpDims D = knock_dims(D0, A.T);
  const size_t sh = knock_lds_bytes(D, KS1);
  const int ntiles = (A.R + 31) >> 5;
  dim3 grid((ntiles + 4 * kTPW - 1) / (4 * kTPW)), block(256);
#define KNOCK_KS(PP, KS) if (KS1 == KS) hipLaunchKernelGGL((k_knock_fwd<PP, KS>), grid, block, sh, st, jobs, A, D);
  if (D.fp32) { KNOCK_KS(PrecF32, 2) KNOCK_KS(PrecF32, 4) }
  else { KNOCK_KS(PrecBF16, 2) KNOCK_KS(PrecBF16, 4) }
#undef KNOCK_KS
  HIP_OK(hipGetLastError());
}

void launch_knock_reduce(const KnockReduceArgs& A, hipStream_t st) {
  if (A.pv.T < 1 || A.pv.T > 65535 || A.K < 1 || A.K > 65535 || A.G < 1 || A.G > 4096 || A.R <= 0)
    dlap_throw_hip(hipErrorInvalidValue, "knockout: unsupported arguments", __FILE__, __LINE__);
  const size_t sh = (size_t)kRW * 5 * sizeof(double) + (size_t)2 * A.G * sizeof(float);
  hipLaunchKernelGGL(k_knock_reduce, dim3((unsigned)A.pv.T, (unsigned)A.K), dim3(kRT), sh, st, A);
  HIP_OK(hipGetLastError());
}
