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
//   k_knock_macro_fill, k_knock_fwd_pp   macro knock-outs (knock.h): the altered series of a
//                    chunk's scenarios, and the tower pass of k_knock_fwd with one per-period
//                    table per (scenario, member) inserted per scenario (described at the kernel).
//                    The same ownership, stores and bits as k_knock_fwd where the table is the
//                    split's own.
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

// ---- macro knock-outs: one per-period table per (scenario, member) ----------------------------
// LDS of k_knock_fwd_pp: [blob | aux] (no per-period inputs), the masks of a full chunk, then the
// current member's table pointers of a full chunk.
MlpDims knock_pp_dims(const MlpDims& D0) {
  MlpDims D = D0;
  D.pp_lds_floats = 0;
  return D;
}
__host__ __device__ inline size_t knock_tab_base(const MlpDims& D, int KS1) { return (knock_lds_bytes(D, KS1) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t knock_pp_lds_bytes(const MlpDims& D, int KS1) {
  return knock_tab_base(D, KS1) + (size_t)KNOCK_MAX_CHUNK * sizeof(const float*);
}

// k_knock_fwd with the [ppc, ppc + Dm) columns of the fragments taken per scenario from the fp32
// table tabs[k][g] ([T][Dm]: the LSTM output, or the macro series themselves, of the scenario's
// altered series). The tile is loaded once per member without the insertion (finish_tile<INS =
// false>); per scenario the characteristic mask is applied as in k_knock_fwd and the lane groups
// whose 8 columns fall into the per-period range take pp[t(row)][c0 .. c0 + 7] with the conversion
// of the forward's staged path (P::pack of the fp32 values, zero beyond Dm), replacing the whole
// fragment where c0 >= 0 and the row is inside R, as finish_tile does.
// The rows are read from global memory (the tables are small and stay in L2; 16-byte loads where
// Dm is a multiple of 4, else 4-byte loads with clamped columns), and the next scenario's rows are
// in flight while the current scenario's tower runs: they are issued right after the current rows
// were packed and waited for at the top of the next iteration. This is the variant that was built
// and measured (profiles/macro_knockout_timing.txt); staging sub-chunks of tables in LDS was not:
// with K * G tables of T * Dm floats each, a sub-chunk would have to be restaged (a barrier and a
// round trip) every few scenarios, while the loads here overlap the MFMAs of a whole tower.
// NS: the trailing k-steps of the row that can hold per-period columns (k-step s holds some iff
// 32 s + 32 > ppc), so only their rows take registers. PRE: the prefetch above; without it (the
// builds the launcher picks where the 8 * 2 * NS fp32 values in flight across a tower would not
// fit the register budget) the rows are loaded where they are packed.
// VEC: Dm is a multiple of 4, so the rows of a table are 16-byte aligned (the tables are, and a
// lane's first column is a multiple of 8): two 16-byte loads per fragment, else eight 4-byte loads.
template <class P, int KS1, int NS, bool PRE, bool VEC>
__global__ __launch_bounds__(256, P::kF32 ? 1 : 2)
void k_knock_fwd_pp(const MlpJob* __restrict__ jobs, KnockPpArgs B, MlpDims D) {
  using Frag = typename P::Frag;
  static_assert(NS >= 1 && NS <= KS1, "per-period k-steps");
  const KnockArgs& A = B.a;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Frag* lds = reinterpret_cast<Frag*>(smem);
  float* aux = aux_lds_ptr(smem, D);
  uint32_t* smask = reinterpret_cast<uint32_t*>(smem + knock_mask_base(D));      // [K][KS1]
  const float** stab = reinterpret_cast<const float**>(smem + knock_tab_base(D, KS1));   // [K]
  const int lane = lane_id(), wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  const int ntiles = (A.R + 31) >> 5;
  const int tile0 = blockIdx.x * (4 * kTPW) + wave;           // this wave's tiles: tile0 + 4 k
  for (int i = threadIdx.x; i < A.K * KS1; i += blockDim.x) smask[i] = gp(A.masks)[i];
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
  const bool ins = D.Dm > 0;
  for (int g = 0; g < A.G; ++g) {
    const MlpJob J = jobs[g];
    DLAP_ASSERT(J.R == A.R && J.T == A.T);
    __syncthreads();                                   // every wave is done with the previous model's image
    if (ins)
      for (int k = threadIdx.x; k < A.K; k += blockDim.x) stab[k] = gp(B.tabs)[(size_t)k * A.G + g];
    stage_weights<P>(J, D, lds, aux);                  // (ends with a barrier: masks and pointers are complete too)
#pragma unroll 1
    for (int kt = 0; kt < kTPW; ++kt) {
      const int tile = tile0 + 4 * kt;
      if (tile >= ntiles) break;                       // wave-uniform; no barrier below
      TileIn<P, KS1> in;
      issue_tile<P, KS1, false>(J, tile, in);          // rows clamped to R - 1
      Frag xf[2][KS1];
      const RowInfo ri = finish_tile<P, KS1, false>(J, D, tile, in, xf);
      const bool okr[2] = {ri.dense[0] >= 0, ri.dense[1] >= 0};
      const int ro[2] = {ri.t[0] * D.Dm, ri.t[1] * D.Dm};       // (clamped rows carry a valid period)
      // the 8 columns of this lane in k-step s start at pp column 32 s + 8 q - ppc
      float raw[2][NS][8];
      // (z: the scenario loop's opaque zero -- the clamped columns and the range predicates are
      // formed per scenario, not kept in registers across the towers)
      auto load_frag = [&](const float* tab, int u, int b, int z) {
        const auto tp = gp(tab);
        const int c0 = 32 * (KS1 - NS + u) + 8 * q - D.ppc + z;
        if constexpr (VEC) {
          const int ca = min(max(c0, 0), D.Dm - 4), cb = min(max(c0 + 4, 0), D.Dm - 4);
          const f32x4 v0 = ld4(tp + ro[b] + ca);
          f32x4 v1 = zero4();
          if (D.Dm > 4) v1 = ld4(tp + ro[b] + cb);
#pragma unroll
          for (int j = 0; j < 4; ++j) { raw[b][u][j] = v0[j]; raw[b][u][4 + j] = v1[j]; }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) raw[b][u][j] = tp[ro[b] + min(max(c0 + j, 0), D.Dm - 1)];
        }
      };
      auto load_rows = [&](const float* tab, int z) {
#pragma unroll
        for (int u = 0; u < NS; ++u)
#pragma unroll
          for (int b = 0; b < 2; ++b) load_frag(tab, u, b, z);
      };
      if (PRE && ins) load_rows(stab[0], 0);
      float* dst = A.wk + (size_t)g * A.R + tile * 32 + n;
      auto store_w = [&](int k, const float (&w)[2]) {
        if (q == 0) {
          float* d = dst + (size_t)k * A.G * A.R;
          if (tile * 32 + n < A.R) *gp(d) = w[0];
          if (tile * 32 + 16 + n < A.R) *gp(d + 16) = w[1];
        }
      };
      float wp[2] = {0.f, 0.f};                        // PRE: the previous scenario's weights
#pragma unroll 1
      for (int k = 0; k < A.K; ++k) {
        const int oz = opaque_zero();                  // no weight fragment kept across scenarios
        const int zc = NS == 1 && VEC ? 0 : oz;        // (one k-step, two loads: columns and predicates stay in registers)
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
        if (ins) {
#pragma unroll
          for (int u = 0; u < NS; ++u) {
            const int s = KS1 - NS + u;
            const int c0 = 32 * s + 8 * q - D.ppc + zc;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              if (!PRE) {                              // one fragment's rows at a time, consumed below
                asm volatile("" ::: "memory");
                load_frag(stab[k], u, b, zc);
              }
              f32x4 lo, hi;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                lo[j] = c0 + j < D.Dm ? raw[b][u][j] : 0.f;
                hi[j] = c0 + 4 + j < D.Dm ? raw[b][u][4 + j] : 0.f;
              }
              const Frag f = P::pack(lo, hi);
              xk[b][s] = (c0 >= 0 && okr[b]) ? f : xk[b][s];
            }
          }
        }
        // (the previous scenario's weights are stored here, ahead of the prefetch: stores and loads
        // share one in-order counter, so a store issued after the loads would be waited for with them)
        if (PRE && k > 0) store_w(k - 1, wp);
        if (PRE && ins) load_rows(stab[min(k + 1, A.K - 1)], zc);   // the next scenario's rows, in flight during the tower

        auto l0 = [&](f32x4 (&a)[2][4]) {
          f32x4 init[2][4];
          bias_init<4>(auxt + D.a_sb, init);
          layer0<P, KS1, 4>(ldt, D.s_fwd0, xk, init, a);
        };
        float w[2];
        sdf_forward_tile<P, false>(ldt, auxt, Dt, kw, l0, w);
        if (PRE) { wp[0] = w[0]; wp[1] = w[1]; }
        else store_w(k, w);
      }
      if (PRE) store_w(A.K - 1, wp);
    }
  }
}

__global__ __launch_bounds__(256) void k_knock_macro_fill(KnockFillArgs a) {
  const int u = blockIdx.y, MW = (a.M + 31) / 32;
  const size_t n = (size_t)a.T * a.M;
  const auto mk = gp(a.masks) + (size_t)u * MW;
  const auto out = gp(a.out) + (size_t)u * a.stride;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % (size_t)a.M);
    const bool rep = (mk[j >> 5] >> (j & 31)) & 1u;
    out[i] = rep ? gp(a.base)[j] : gp(a.macro)[i];
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

bool knock_pp_supported(const MlpDims& D0, int KS1, int T) {
  return knock_supported(D0, KS1, T) && knock_pp_lds_bytes(knock_pp_dims(D0), KS1) <= 160 * 1024;
}

void launch_knock_fwd_pp(const MlpJob* jobs, const KnockPpArgs& B, const MlpDims& D0, int KS1, hipStream_t st) {
  const KnockArgs& A = B.a;
  if (!knock_pp_supported(D0, KS1, A.T) || A.R <= 0 || A.G <= 0 || A.K < 1 || A.K > KNOCK_MAX_CHUNK ||
      (D0.Dm > 0 && !B.tabs))
    dlap_throw_hip(hipErrorInvalidValue, "knockout_macro: unsupported shape", __FILE__, __LINE__);
  const MlpDims D = knock_pp_dims(D0);
  const size_t sh = knock_pp_lds_bytes(D, KS1);
  const int ntiles = (A.R + 31) >> 5;
  dim3 grid((ntiles + 4 * kTPW - 1) / (4 * kTPW)), block(256);
  // the trailing k-steps with per-period columns (header of k_knock_fwd_pp); none with Dm = 0
  const int NS = std::max(1, KS1 - D.ppc / 32);
  // (the build without the prefetch keeps to the 4-byte loads: its register budget)
  const bool vec = D.Dm > 0 && (D.Dm & 3) == 0;
#define KNOCK_PP1(PP, KS, N, PRE, VEC) hipLaunchKernelGGL((k_knock_fwd_pp<PP, KS, N, PRE, VEC>), grid, block, sh, st, jobs, B, D);
#define KNOCK_PP(PP, KS, N) if (vec) { KNOCK_PP1(PP, KS, N, true, true) } else { KNOCK_PP1(PP, KS, N, true, false) }
  if (D.fp32) {
    if (KS1 == 2) { if (NS == 1) { KNOCK_PP(PrecF32, 2, 1) } else { KNOCK_PP(PrecF32, 2, 2) } }
    else if (NS == 1) { KNOCK_PP(PrecF32, 4, 1) } else if (NS == 2) { KNOCK_PP(PrecF32, 4, 2) }
    else { KNOCK_PP1(PrecF32, 4, 4, false, false) }
  } else {          // (128-column bf16 rows: two waves per SIMD leave room for one k-step's rows in flight)
    if (KS1 == 2) { if (NS == 1) { KNOCK_PP(PrecBF16, 2, 1) } else { KNOCK_PP(PrecBF16, 2, 2) } }
    else if (NS == 1) { KNOCK_PP(PrecBF16, 4, 1) } else { KNOCK_PP1(PrecBF16, 4, 4, false, false) }
  }
#undef KNOCK_PP1
#undef KNOCK_PP
  HIP_OK(hipGetLastError());
}

void launch_knock_macro_fill(const KnockFillArgs& A, hipStream_t st) {
  if (A.U < 1 || A.U > 65535 || A.T < 1 || A.M < 1 || (A.stride & 3) || A.stride < (size_t)A.T * A.M)
    dlap_throw_hip(hipErrorInvalidValue, "knockout_macro: unsupported arguments", __FILE__, __LINE__);
  const size_t n = (size_t)A.T * A.M;
  const unsigned gx = (unsigned)std::min<size_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(k_knock_macro_fill, dim3(gx, (unsigned)A.U), dim3(256), 0, st, A);
  HIP_OK(hipGetLastError());
}

void launch_knock_reduce(const KnockReduceArgs& A, hipStream_t st) {
  if (A.pv.T < 1 || A.pv.T > 65535 || A.K < 1 || A.K > 65535 || A.G < 1 || A.G > 4096 || A.R <= 0)
    dlap_throw_hip(hipErrorInvalidValue, "knockout: unsupported arguments", __FILE__, __LINE__);
  const size_t sh = (size_t)kRW * 5 * sizeof(double) + (size_t)2 * A.G * sizeof(float);
  hipLaunchKernelGGL(k_knock_reduce, dim3((unsigned)A.pv.T, (unsigned)A.K), dim3(kRT), sh, st, A);
  HIP_OK(hipGetLastError());
}
