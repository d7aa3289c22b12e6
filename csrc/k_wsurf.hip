// SDF weight structure: response curves and interaction surfaces of the raw SDF weight (definition
// in wsurf.h). An analysis pass beside the training kernels: nothing here runs inside an epoch graph.
//
// Reference op: `SDFNetwork.forward` in evaluation mode on generated feature rows -- the base row
// with one (curve) or two (surface) characteristics replaced by grid values -- in every period of
// a split, weighted by s[g][t] and summed over periods and models.
//
// The rows are never in memory. A 32-row tile (T orientation of k_mlp.hip) is the X operand of
// layer 0, lane (q, n) holding columns 32 s + 8 q + j of row n: the row index decodes to
// (item, p, q) by arithmetic, and the lane sets base[col], or u[p] / u[q] at the item's columns,
// with the conversion the panel upload uses (P::set). That characteristic part is built once per
// wave and kept in registers. The period enters through the [ppc, ppc + Dm) columns only, the same
// for every row: per period one fragment per k-step is packed from the LDS copy of pp_g[t] exactly
// as finish_tile does and selected into the lanes that own those columns. The tile then runs the
// forward's own layer0 / sdf_forward_tile on the staged evaluation blob, so a row's raw weight has
// the bits forward_split gives a real stock with that feature row in that period.
//
// Model-outer: for each model the workgroup stages the blob, aux, pp_g [T][ppst] and the model's T
// scales, and wave 0 compacts the periods with a non-zero scale into an ordered list (the others
// are skipped). Each row has one fp32 accumulator, acc = fma(s[g][t], w, acc), g outer and t
// inner in list order: the order depends on nothing else (not on the chunking below, the grid, the
// row's position or the other items). No atomics; one lane stores each row once.
//
// Chunking (host's choice, by the number of tiles against the device's SIMDs):
//   PS = 1  a wave owns TPW tiles (wave w: tiles 4 k + w of the workgroup's 4 TPW) and walks the
//           list alone -- no barrier inside a model;
//   PS > 1  few tiles: PS waves share one tile. Round i, wave j evaluates the kEPW list entries
//           (i PS + j) kEPW + b and leaves their scales and 32 weights each in LDS (double-buffered,
//           one barrier per round); then every wave of the tile adds the round's PS kEPW weights to
//           its accumulator in list order. Only the tower evaluations run in parallel: the fma
//           sequence of a row is the one of PS = 1.
#include <algorithm>
#include "common.h"
#include "layout.h"
#include "mlp.h"
#include "tower_dev.h"
#include "wsurf.h"

namespace {

constexpr int kEPW = 4;              // list entries a wave evaluates per round when waves share a tile
constexpr int kWRow = 33;            // exchange record: 32 weights + the period's scale

// launch dims: the periods' inputs are always staged (T of the split), whatever the engine's
// tower kernels do for their largest split
MlpDims wsurf_dims(const MlpDims& D0, int T) {
  MlpDims D = D0;
  D.pp_lds_floats = D0.Dm > 0 ? T * D0.ppst : 0;
  return D;
}
// LDS image: [blob | aux | pp] (tower_dev.h), then scales [T], live periods [T] + their count,
// then the exchange buffer [2][8 waves][kEPW][kWRow]
__host__ __device__ inline size_t wsurf_scale_base(const MlpDims& D) { return (lds_bytes_of(D) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t wsurf_wbuf_base(const MlpDims& D, int T) {
  return (wsurf_scale_base(D) + (size_t)(2 * T + 1) * 4 + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t wsurf_lds_bytes(const MlpDims& D, int T) {
  return wsurf_wbuf_base(D, T) + (size_t)2 * 8 * kEPW * kWRow * sizeof(float);
}

// Characteristic part of the X fragments of rows r (one per row block), clamped by the caller.
template <class P, int KS1>
DLAP_DEV void build_rows(const WsurfArgs& A, const int (&r)[2], typename P::Frag (&xf)[2][KS1]) {
  const int q = lane_id() >> 4;
  const int PP = A.P * A.P, nc = A.n1 * A.P;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    int item, ip, iq;
    if (r[b] < nc) {
      item = r[b] / A.P; ip = r[b] - item * A.P; iq = 0;
    } else {
      const int rr = r[b] - nc, it = rr / PP, rem = rr - it * PP;
      item = A.n1 + it; ip = rem / A.P; iq = rem - ip * A.P;
    }
    const int2 ab = gp(A.items)[item];
    const float ua = gp(A.grid)[ip], ub = gp(A.grid)[iq];
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
      const int c0 = 32 * s + 8 * q;
      const f32x4 lo = ld4(gp(A.base) + c0), hi = ld4(gp(A.base) + c0 + 4);
      typename P::Frag f = P::zero();
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = j < 4 ? lo[j & 3] : hi[j & 3];
        v = (c0 + j == ab.x) ? ua : v;
        v = (c0 + j == ab.y) ? ub : v;
        P::set(f, j, v);
      }
      xf[b][s] = f;
    }
  }
}

DLAP_DEV int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
DLAP_DEV float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <class P, int KS1, int PS, int TPW>
__global__ __launch_bounds__(PS == 8 ? 512 : 256, (PS == 8 || !P::kF32) ? 2 : 1)
void k_wsurf(const MlpJob* __restrict__ jobs, WsurfArgs A, MlpDims D) {
  static_assert(PS == 1 || TPW == 1, "shared tiles are one per wave group");
  using Frag = typename P::Frag;
  constexpr int NW = PS == 8 ? 8 : 4, SLOTS = NW / PS;        // tile slots of the workgroup per k
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Frag* lds = reinterpret_cast<Frag*>(smem);
  float* aux = aux_lds_ptr(smem, D);
  float* spp = pp_lds_ptr(smem, D);
  float* ssc = reinterpret_cast<float*>(smem + wsurf_scale_base(D));
  int* live = reinterpret_cast<int*>(ssc + A.T);               // [T] periods with a non-zero scale, [T] = count
  float* wbuf = reinterpret_cast<float*>(smem + wsurf_wbuf_base(D, A.T));
  const int lane = lane_id(), wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  const int slot = wave / PS, pl = wave % PS;
  const int tile0 = blockIdx.x * (SLOTS * TPW) + slot;        // this wave's tiles: tile0 + SLOTS k
  Frag xc[TPW][2][KS1];
  float acc[TPW][2];
  bool on[TPW];
#pragma unroll
  for (int k = 0; k < TPW; ++k) {
    const int r0 = (tile0 + SLOTS * k) * 32;
    on[k] = r0 < A.rows;                                      // wave-uniform
    const int r[2] = {min(r0 + n, A.rows - 1), min(r0 + 16 + n, A.rows - 1)};
    build_rows<P, KS1>(A, r, xc[k]);
    acc[k][0] = acc[k][1] = 0.f;
  }
  const uint32_t kw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  for (int g = 0; g < A.G; ++g) {
    const MlpJob J = jobs[g];
    DLAP_ASSERT(J.T == A.T);
    __syncthreads();                                   // every wave is done with the previous model's image
    for (int t = threadIdx.x; t < A.T; t += blockDim.x) ssc[t] = gp(A.scale)[(size_t)g * A.T + t];
    stage_weights<P>(J, D, lds, aux, spp);             // (ends with a barrier: the scales are complete too)
    if (wave == 0) {
      int cnt = 0;
      for (int t0 = 0; t0 < A.T; t0 += 64) {
        const int t = t0 + lane;
        const bool nz = t < A.T && ssc[t] != 0.f;
        const unsigned long long m = __ballot(nz);
        if (nz) live[cnt + __popcll(m & ((1ull << lane) - 1ull))] = t;
        cnt += __popcll(m);
      }
      if (lane == 0) live[A.T] = cnt;
    }
    __syncthreads();
    const int nlive = uniform(live[A.T]);
    constexpr int EPW = PS == 1 ? 1 : kEPW;
    const int rounds = (nlive + PS * EPW - 1) / (PS * EPW);
    for (int i = 0; i < rounds; ++i) {
#pragma unroll 1
      for (int bb = 0; bb < EPW; ++bb) {
        const int idx = (i * PS + pl) * EPW + bb;
        if (idx >= nlive) break;                       // wave-uniform
        const int t = uniform(live[idx]);
        const float sc = uniform(ssc[t]);
        // the period's columns, as finish_tile inserts them from the LDS copy
        Frag pf[KS1];
        if (D.Dm > 0) {
#pragma unroll
          for (int s = 0; s < KS1; ++s) {
            if (32 * s + 32 <= D.ppc) continue;                 // wave-uniform
            const int c0 = 32 * s + 8 * q - D.ppc;
            const float* row = spp + t * D.ppst;
            const int ca = min(max(c0, 0), D.ppst - 4), cb = min(max(c0 + 4, 0), D.ppst - 4);
            const f32x4 v0 = ld4(row + ca), v1 = ld4(row + cb);
            pf[s] = P::pack(v0, c0 + 4 < D.ppst ? v1 : zero4());
          }
        }
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
          if (!on[k]) continue;
          const int oz = opaque_zero();                // no weight fragment kept across tiles
          const Frag* ldt = lds + oz;
          const float* auxt = aux + oz;
          MlpDims Dt = D;
          Dt.nl_sdf += oz;
          Frag xf[2][KS1];
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < KS1; ++s) {
              xf[b][s] = xc[k][b][s];
              if (D.Dm > 0 && 32 * s + 32 > D.ppc) xf[b][s] = (32 * s + 8 * q - D.ppc >= 0) ? pf[s] : xf[b][s];
            }
          auto l0 = [&](f32x4 (&a)[2][4]) {
            f32x4 init[2][4];
            bias_init<4>(auxt + D.a_sb, init);
            layer0<P, KS1, 4>(ldt, D.s_fwd0, xf, init, a);
          };
          float w[2];
          sdf_forward_tile<P, false>(ldt, auxt, Dt, kw, l0, w);
          if constexpr (PS == 1) {
            acc[k][0] = __builtin_fmaf(sc, w[0], acc[k][0]);
            acc[k][1] = __builtin_fmaf(sc, w[1], acc[k][1]);
          } else if (q == 0) {
            float* dst = wbuf + (((i & 1) * NW + wave) * EPW + bb) * kWRow;
            dst[n] = w[0];
            dst[16 + n] = w[1];
            if (n == 0) dst[32] = sc;
          }
        }
      }
      if constexpr (PS > 1) {
        __syncthreads();                               // the round's weights are in LDS (and the
                                                       // buffer of round i - 1 is free for round i + 1)
        // the slot's records of this round are consecutive in list order; loads unconditional (a
        // record beyond the list holds stale values), the fma only for the list's entries
        const float* src = wbuf + ((i & 1) * NW + slot * PS) * EPW * kWRow;
        const int left = nlive - i * PS * EPW;
#pragma unroll
        for (int j = 0; j < PS * EPW; ++j) {
          const float s2 = src[j * kWRow + 32], w0 = src[j * kWRow + n], w1 = src[j * kWRow + 16 + n];
          acc[0][0] = j < left ? __builtin_fmaf(s2, w0, acc[0][0]) : acc[0][0];
          acc[0][1] = j < left ? __builtin_fmaf(s2, w1, acc[0][1]) : acc[0][1];
        }
      }
    }
  }
  if (pl == 0) {
#pragma unroll
    for (int k = 0; k < TPW; ++k)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int r = (tile0 + SLOTS * k) * 32 + 16 * b + n;
        if (q == 0 && r < A.rows) gp(A.out)[r] = acc[k][b];
      }
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
bool wsurf_supported(const MlpDims& D0, int KS1, int T) {
  if (D0.wide || (KS1 != 2 && KS1 != 4) || T < 1) return false;
  if (D0.nl_sdf < 1 || D0.nl_sdf > 4) return false;
  if (D0.F + D0.Dm > 32 * KS1 || D0.ppc < D0.F || D0.ppc + D0.Dm > 32 * KS1) return false;
  return wsurf_lds_bytes(wsurf_dims(D0, T), T) <= 160 * 1024;
}

WsurfPlan launch_weight_surface(const MlpJob* jobs, const WsurfArgs& A, const MlpDims& D0, int KS1, hipStream_t st) {
  if (!wsurf_supported(D0, KS1, A.T) || A.rows <= 0 || A.G <= 0 || A.P < 2 || A.P > WSURF_MAX_P)
    dlap_throw_hip(hipErrorInvalidValue, "weight_surface: unsupported shape", __FILE__, __LINE__);
  const MlpDims D = wsurf_dims(D0, A.T);
  const size_t sh = wsurf_lds_bytes(D, A.T);
  const int ntiles = (A.rows + 31) >> 5;
  // Rows are the only parallel axis a wave can own alone. With fewer tiles than SIMDs, PS waves
  // share a tile (the smallest PS in {2, 4, 8} that gives every SIMD a wave, else 8); with four
  // tiles or more per SIMD a wave takes two. The sums do not depend on the choice.
  int dev = 0, cus = 0;
  HIP_OK(hipGetDevice(&dev));
  HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const long long simds = 4ll * std::max(cus, 1);
  WsurfPlan pl{1, 1};
  if (ntiles >= 4 * simds) pl.tiles_per_wave = 2;
  else if (ntiles < simds) pl.period_split = 2ll * ntiles >= simds ? 2 : (4ll * ntiles >= simds ? 4 : 8);
  const int ps = pl.period_split, tpw = pl.tiles_per_wave;
  const int per_wg = (ps == 8 ? 1 : 4 / ps) * tpw;
  dim3 grid((ntiles + per_wg - 1) / per_wg), block(ps == 8 ? 512 : 256);
#define WSURF_CFG(PP, KS, S, N) if (ps == S && tpw == N) \
    hipLaunchKernelGGL((k_wsurf<PP, KS, S, N>), grid, block, sh, st, jobs, A, D);
#define WSURF_KS(PP, KS) if (KS1 == KS) { \
    WSURF_CFG(PP, KS, 1, 1) WSURF_CFG(PP, KS, 1, 2) WSURF_CFG(PP, KS, 2, 1) WSURF_CFG(PP, KS, 4, 1) WSURF_CFG(PP, KS, 8, 1) }
  if (D.fp32) { WSURF_KS(PrecF32, 2) WSURF_KS(PrecF32, 4) }
  else { WSURF_KS(PrecBF16, 2) WSURF_KS(PrecBF16, 4) }
#undef WSURF_KS
#undef WSURF_CFG
  HIP_OK(hipGetLastError());
  return pl;
}
