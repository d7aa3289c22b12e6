// Cross-sectional factor imputation on a ranked chunk (ximpute.h).
//
//   k_ximp_gram   grid (super-tiles, periods), 256 threads. A workgroup owns one period and one
//             super-tile (ia, ib), ia <= ib, of the ceil(F / 64)^2 grid of 64 x 64 column blocks; wave
//             w owns the 16 columns 64 ia + 16 w .. + 15 against the four 16-column blocks of ib, of
//             which the tiles with a <= b are computed. The workgroup walks the period's stocks in
//             stages of 64 (two MFMA steps of 32): the 256 threads read the 64 (ia == ib) or 128
//             columns of the stage's rows (4, 2 or 1 floats per load, as F and the chunk's alignment
//             allow; the next stage's loads are in flight during a stage's MFMAs) and write two
//             LDS images, z (fp32; the select-to-zero applied: hole, dead row, stock >= N, column
//             >= F) and the indicator o (bf16 1 / 0).
//             The stocks are the MFMA k axis, so the operand is the transpose of the stored rows
//             (k_xgram's scheme): lane (q, n) holds column n of rows 8 q + j,
//               z   eight v_mfma_f32_16x16x4_f32 per tile and step, fragments by ds_read_b32;
//               o   one v_mfma_f32_16x16x32_bf16, fragments by two ds_read_b64_tr_b16.
//             After every XIMP_RUN stocks the fp32 tiles join the fp64 sums (z) and the int32
//             counts (o) the wave keeps in registers. At the end a lane writes its C-layout
//             elements and their mirror images; of a diagonal tile only i <= j.
//   k_ximp_fill<K>   grid (ceil(N / 256), periods), 256 threads; a wave owns 64 rows. The period's
//             table [F rounded up to 32][lam_f (K) | vech(lam_f lam_f') (K (K + 1) / 2) | 0] sits in
//             LDS. Both accumulations are fp32 MFMA GEMMs with the rows as the m axis and the
//             characteristics as the k axis: b = Z . lam and vech(A) - gamma I = O . P; the A operand
//             comes straight from the row in global memory (lane (q, m): columns 32 s + 8 q + j of
//             row m, selected), the B operand from the table. The wave transposes the results
//             through LDS so that lane l holds row l, solves the K x K system by Cholesky in
//             registers (fp32) and leaves g in LDS; then the 64 lanes walk the wave's 64 F
//             elements in memory order and write clip(lam_f . g) into the holes (and, out of place,
//             copy everything else).
// Every loop is bounded by N, F or K; every global index is clamped into the caller's buffers
// before the load and the value selected afterwards.
#include <algorithm>
#include "common.h"
#include "ximpute.h"

namespace {

constexpr int kNT = 256;
constexpr int kStep = 32;                      // stocks of an MFMA step (the bf16 MFMA's k)
constexpr int kStage = 64;                     // stocks staged per barrier pair
constexpr int kZS = 134;                       // floats of a z image row: 128 columns + 6 (8 rows apart: 48 banks)
constexpr int kOS = 272;                       // bytes of an o image row: 128 bf16 + 16
constexpr size_t kGramLds = (size_t)kStage * kZS * sizeof(float) + (size_t)kStage * kOS;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
#define LDS3 __attribute__((address_space(3)))

struct XimpGramArgs {
  const float* y;           // [periods][N][F]
  const uint8_t* rowok;     // [periods][N]
  double* S;                // [periods][F][F]
  int* C;                   // [periods][F][F]
  int N, F;
};

// z fragment of the 16-column block `slot`: lane (q, n) <- column n of rows 8 q + j
DLAP_DEV f32x8 zfrag(const float* img, int slot, int q, int n) {
  const float* p = img + (8 * q) * kZS + slot * 16 + n;
  f32x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = p[j * kZS];
  return f;
}
// o fragment: the transposed read, the lane supplies row 8 q + (n >> 2), columns 4 (n & 3) .. + 3 of the block
DLAP_DEV bf16x8 ofrag(const char* img, int slot, int q, int n) {
  char* p = const_cast<char*>(img) + (8 * q + (n >> 2)) * kOS + slot * 32 + (n & 3) * 8;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS3 s16x4*)p);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS3 s16x4*)(p + 4 * kOS));
  const s16x8 v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// V = 4, 2, 1: floats of a staging load (the launcher: V divides F and the chunk is V-float aligned)
template <int V>
__global__ __launch_bounds__(kNT) void k_ximp_gram(XimpGramArgs a) {
  constexpr int LV = V == 4 ? 2 : V == 2 ? 1 : 0;
  constexpr int kIT = kStage * 128 / (kNT * V);                               // staging loads of a thread at most
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* zimg = reinterpret_cast<float*>(smem);                              // [kStage][kZS]
  char* oimg = smem + (size_t)kStage * kZS * sizeof(float);                  // [kStage][kOS]
  const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, n = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, F = a.F, NB = (F + 15) >> 4;
  int ib = 0, ia = (int)blockIdx.x;                                          // super-tiles ordered by ib, then ia <= ib
  while (ia > ib) { ia -= ib + 1; ++ib; }
  const bool diag = ia == ib;
  const int lnc = diag ? 6 : 7;                                              // log2 of the staged columns: the blocks of ia, then ib's
  const size_t t = blockIdx.y;
  const DLAP_GLOBAL float* y = gp(a.y) + t * (size_t)N * F;
  const DLAP_GLOBAL uint8_t* rok = gp(a.rowok) + t * (size_t)N;

  const int ba = 4 * ia + w, sb0 = diag ? 0 : 4;
  bool okt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) okt[j] = ba < NB && 4 * ib + j < NB && ba <= 4 * ib + j;

  f32x4 acc[4], cac[4];
  double sum[4][4];
  int cnt[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = zero4();
    cac[j] = zero4();
#pragma unroll
    for (int r = 0; r < 4; ++r) { sum[j][r] = 0.0; cnt[j][r] = 0; }
  }

  // Staging: a thread owns V adjacent image columns c .. and the rows rw0, rw0 + rstep, .. of a stage.
  // The loads of stage s + 1 are issued into registers before the MFMAs of stage s and written to the
  // images after them, so a workgroup does not wait on memory between its stages.
  const int lgr = lnc - LV, rw0 = tid >> lgr, rstep = kNT >> lgr, nit = kStage / rstep;
  const int c = (tid & ((1 << lgr) - 1)) * V;
  const int col = c < 64 ? 64 * ia + c : 64 * ib + (c - 64);
  const bool colok = col < F;                                   // (V divides F: then col + V - 1 < F too)
  const DLAP_GLOBAL float* ycol = y + (colok ? col : 0);        // (a clamped element re-reads a live one)
  float pv[kIT][V];
  bool pk[kIT];
  auto fetch = [&](int s0) {
#pragma unroll
    for (int i = 0; i < kIT; ++i)
      if (i < nit) {
        const int stock = s0 + rw0 + i * rstep, si = min(stock, N - 1);
        pk[i] = stock < N && colok && rok[si] != 0;
        const DLAP_GLOBAL float* p = ycol + (size_t)si * F;
        if constexpr (V == 4) {
          const f32x4 v = *reinterpret_cast<const DLAP_GLOBAL f32x4*>(p);
          pv[i][0] = v[0]; pv[i][1] = v[1]; pv[i][2] = v[2]; pv[i][3] = v[3];
        } else if constexpr (V == 2) {
          const f32x2 v = *reinterpret_cast<const DLAP_GLOBAL f32x2*>(p);
          pv[i][0] = v[0]; pv[i][1] = v[1];
        } else {
          pv[i][0] = *p;
        }
      }
  };
  auto commit = [&]() {                                         // every row of the stage: a stock >= N is zero
#pragma unroll
    for (int i = 0; i < kIT; ++i)
      if (i < nit) {
        const int row = rw0 + i * rstep;
        float z[V];
        u16 o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const bool obs = pk[i] && pv[i][e] == pv[i][e];
          z[e] = obs ? pv[i][e] : 0.f;
          o[e] = obs ? (u16)0x3F80u : (u16)0u;
        }
        float* zp = zimg + row * kZS + c;                       // (8-byte aligned for V >= 2: kZS is even)
        char* op = oimg + row * kOS + c * 2;
        if constexpr (V == 4) {
          *reinterpret_cast<f32x2*>(zp) = f32x2{z[0], z[1]};
          *reinterpret_cast<f32x2*>(zp + 2) = f32x2{z[2], z[3]};
          *reinterpret_cast<uint2*>(op) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
        } else if constexpr (V == 2) {
          *reinterpret_cast<f32x2*>(zp) = f32x2{z[0], z[1]};
          *reinterpret_cast<uint32_t*>(op) = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
        } else {
          *zp = z[0];
          *reinterpret_cast<u16*>(op) = o[0];
        }
      }
  };

  const int nstage = (N + kStage - 1) / kStage;
  fetch(0);
  for (int s = 0; s < nstage; ++s) {
    __syncthreads();                                            // (the previous stage's reads are done)
    commit();
    __syncthreads();
    if (s + 1 < nstage) fetch((s + 1) * kStage);
    const int nsub = min(kStage / kStep, (N - s * kStage + kStep - 1) / kStep);
    if (ba < NB) {
      for (int sub = 0; sub < nsub; ++sub) {
        const float* zi = zimg + sub * kStep * kZS;
        const char* oi = oimg + sub * kStep * kOS;
        const f32x8 za = zfrag(zi, w, q, n);
        const bf16x8 oa = ofrag(oi, w, q, n);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (okt[j]) {
            acc[j] = PrecF32::mma(za, zfrag(zi, sb0 + j, q, n), acc[j]);
            cac[j] = mfma16(oa, ofrag(oi, sb0 + j, q, n), cac[j]);
          }
      }
    }
    if (((s + 1) * kStage) % XIMP_RUN != 0 && s + 1 != nstage) continue;      // a run of XIMP_RUN stocks ends here
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                 // the run's fp32 tiles join the fp64 sums and the counts
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sum[j][r] += (double)acc[j][r];
        cnt[j][r] += (int)cac[j][r];
      }
      acc[j] = zero4();
      cac[j] = zero4();
    }
  }

  DLAP_GLOBAL double* S = gp(a.S) + t * (size_t)F * F;
  DLAP_GLOBAL int* C = gp(a.C) + t * (size_t)F * F;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!okt[j]) continue;
    const int gj = 16 * (4 * ib + j) + n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                 // C layout: rows 4 q + r, column n
      const int gi = 16 * ba + 4 * q + r;
      if (gi >= F || gj >= F || gi > gj) continue;                // (gi > gj: a diagonal tile's lower half)
      S[(size_t)gi * F + gj] = sum[j][r];
      C[(size_t)gi * F + gj] = cnt[j][r];
      if (gi != gj) {
        S[(size_t)gj * F + gi] = sum[j][r];
        C[(size_t)gj * F + gi] = cnt[j][r];
      }
    }
  }
}

struct XimpFillArgs {
  const float* y;           // [periods][N][F]
  const uint8_t* rowok;     // [periods][N]
  const float* lam;         // [periods][F][K]
  float* out;               // [periods][N][F] (may be y)
  int N, F;
  float gamma;
};

template <int K>
__global__ __launch_bounds__(kNT) void k_ximp_fill(XimpFillArgs a) {
  constexpr int NV = K + K * (K + 1) / 2;      // b, then vech(A) row by row (i, j <= i)
  constexpr int NBK = (NV + 15) / 16;          // 16-column blocks of the table
  constexpr int NC = 16 * NBK, TS = NC + 2, XS = NC + 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, n = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, F = a.F, Fp = (F + 31) & ~31;
  float* tab = reinterpret_cast<float*>(smem);                   // [Fp][TS]
  float* xw = tab + (size_t)Fp * TS + w * 64 * XS;               // [64][XS], the wave's own
  const size_t t = blockIdx.y;
  const DLAP_GLOBAL float* y = gp(a.y) + t * (size_t)N * F;
  DLAP_GLOBAL float* out = gp(a.out) + t * (size_t)N * F;
  const DLAP_GLOBAL uint8_t* rok = gp(a.rowok) + t * (size_t)N;
  const DLAP_GLOBAL float* lam = gp(a.lam) + t * (size_t)F * K;

  for (int f = tid; f < Fp; f += kNT) {                          // the period's table; rows >= F are zero
    float l[K];
#pragma unroll
    for (int k = 0; k < K; ++k) l[k] = f < F ? lam[(size_t)min(f, F - 1) * K + k] : 0.f;
    float* r = tab + f * TS;
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = l[k];
    int c = K;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) r[c++] = l[i] * l[j];
#pragma unroll
    for (int cc = NV; cc < NC; ++cc) r[cc] = 0.f;
  }
  __syncthreads();

  const int row0 = blockIdx.x * kNT + w * 64;                    // the wave's rows row0 .. row0 + 63
  f32x4 accb[4], acca[4][NBK];
  const DLAP_GLOBAL float* yr[4];
  bool live[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    const int rr = row0 + 16 * mb + n, ri = min(rr, N - 1);      // (a clamped row re-reads a live one: selected away)
    live[mb] = rr < N && rok[ri] != 0;
    yr[mb] = y + (size_t)ri * F;
    accb[mb] = zero4();
#pragma unroll
    for (int c = 0; c < NBK; ++c) acca[mb][c] = zero4();
  }
  for (int f0 = 8 * q; f0 < Fp; f0 += 32) {                      // lane (q, m): columns f0 .. f0 + 7 of row m
    f32x8 bf[NBK];
#pragma unroll
    for (int c = 0; c < NBK; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) bf[c][j] = tab[(f0 + j) * TS + 16 * c + n];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      f32x8 zf, of;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = yr[mb][min(f0 + j, F - 1)];
        const bool obs = live[mb] && f0 + j < F && v == v;
        zf[j] = obs ? v : 0.f;
        of[j] = obs ? 1.f : 0.f;
      }
      accb[mb] = PrecF32::mma(zf, bf[0], accb[mb]);
#pragma unroll
      for (int c = 0; c < NBK; ++c) acca[mb][c] = PrecF32::mma(of, bf[c], acca[mb][c]);
    }
  }
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)                                 // C layout: rows 4 q + r, column n -> [row][column]
#pragma unroll
    for (int c = 0; c < NBK; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        xw[(16 * mb + 4 * q + r) * XS + 16 * c + n] = (c == 0 && n < K) ? accb[mb][r] : acca[mb][c][r];
  __syncthreads();

  {                                                              // lane l: row row0 + l
    const float* v = xw + lane * XS;
    float L[K][K], inv[K], g[K];
    int c = K;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) L[i][j] = v[c++] + (i == j ? a.gamma : 0.f);
#pragma unroll
    for (int i = 0; i < K; ++i) g[i] = v[i];
#pragma unroll
    for (int i = 0; i < K; ++i)                                  // A = L L'
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        float s = L[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
        if (i == j) {
          L[i][i] = sqrtf(s);
          inv[i] = 1.f / L[i][i];
        } else {
          L[i][j] = s * inv[j];
        }
      }
#pragma unroll
    for (int i = 0; i < K; ++i) {                                // L u = b
      float s = g[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i][k] * g[k];
      g[i] = s * inv[i];
    }
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {                           // L' g = u
      float s = g[i];
#pragma unroll
      for (int k = i + 1; k < K; ++k) s -= L[k][i] * g[k];
      g[i] = s * inv[i];
    }
    float* gw = xw + lane * XS;
#pragma unroll
    for (int k = 0; k < K; ++k) gw[k] = g[k];
  }
  __syncthreads();

  const bool copy = a.out != a.y;
  const int nrow = min(64, N - row0);                            // (<= 0: nothing to write)
  const size_t base = (size_t)row0 * F;
  for (int r = 0, e = lane; r < nrow; ++r) {                     // the wave's elements in memory order
    const bool okr = rok[row0 + r] != 0;
    for (; e < (r + 1) * F; e += 64) {
      const int f = e - r * F;
      const float v = y[base + e];
      if (okr && v != v) {
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) d = fmaf(tab[f * TS + k], xw[r * XS + k], d);
        out[base + e] = fminf(fmaxf(d, -0.5f), 0.5f);
      } else if (copy) {
        out[base + e] = v;
      }
    }
  }
}

template <int K>
void launch_fill_k(const XimpFillArgs& a0, const float* y, const uint8_t* rowok, const float* lam, float* out,
                   long long T, hipStream_t st) {
  XimpFillArgs a = a0;
  const size_t lds = ximp_fill_lds(a.F, K);
  if (lds > 64 * 1024) {                                         // (idempotent; more than the default limit)
    static bool raised = false;
    if (!raised) {
      HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ximp_fill<K>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 XIMP_LDS_MAX));
      raised = true;
    }
  }
  const unsigned gx = (unsigned)((a.N + kNT - 1) / kNT);
  for (long long t0 = 0; t0 < T; t0 += 65535) {
    const long long tc = std::min<long long>(65535, T - t0);
    a.y = y + (size_t)t0 * a.N * a.F;
    a.out = out + (size_t)t0 * a.N * a.F;
    a.rowok = rowok + (size_t)t0 * a.N;
    a.lam = lam + (size_t)t0 * a.F * K;
    hipLaunchKernelGGL(k_ximp_fill<K>, dim3(gx, (unsigned)tc), dim3(kNT), lds, st, a);
    HIP_OK(hipGetLastError());
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
int ximp_run() { return XIMP_RUN; }

void launch_ximp_gram(const float* y, const uint8_t* rowok, double* S, int* C, long long T, int N, int F,
                      hipStream_t st) {
  if (!ximp_supported(F, 1) || N < 1 || T < 0 || !y || !rowok || !S || !C)
    dlap_throw_hip(hipErrorInvalidValue, "ximp_gram: unsupported arguments", __FILE__, __LINE__);
  XimpGramArgs a{};
  a.N = N; a.F = F;
  const int ns = (F + 63) / 64;
  const unsigned gx = (unsigned)(ns * (ns + 1) / 2);
  for (long long t0 = 0; t0 < T; t0 += 65535) {
    const long long tc = std::min<long long>(65535, T - t0);
    a.y = y + (size_t)t0 * N * F;
    a.rowok = rowok + (size_t)t0 * N;
    a.S = S + (size_t)t0 * F * F;
    a.C = C + (size_t)t0 * F * F;
    const uintptr_t al = reinterpret_cast<uintptr_t>(a.y);       // (the bits do not depend on the load width)
    if (F % 4 == 0 && al % 16 == 0) hipLaunchKernelGGL(k_ximp_gram<4>, dim3(gx, (unsigned)tc), dim3(kNT), kGramLds, st, a);
    else if (F % 2 == 0 && al % 8 == 0) hipLaunchKernelGGL(k_ximp_gram<2>, dim3(gx, (unsigned)tc), dim3(kNT), kGramLds, st, a);
    else hipLaunchKernelGGL(k_ximp_gram<1>, dim3(gx, (unsigned)tc), dim3(kNT), kGramLds, st, a);
    HIP_OK(hipGetLastError());
  }
}

void launch_ximp_fill(const float* y, const uint8_t* rowok, const float* lam, float* out, long long T, int N,
                      int F, int K, float gamma, hipStream_t st) {
  if (!ximp_supported(F, K) || N < 1 || T < 0 || !(gamma > 0.f) || !y || !rowok || !lam || !out)
    dlap_throw_hip(hipErrorInvalidValue, "ximp_fill: unsupported arguments", __FILE__, __LINE__);
  XimpFillArgs a{};
  a.N = N; a.F = F; a.gamma = gamma;
  switch (K) {
    case 1: launch_fill_k<1>(a, y, rowok, lam, out, T, st); break;
    case 2: launch_fill_k<2>(a, y, rowok, lam, out, T, st); break;
    case 3: launch_fill_k<3>(a, y, rowok, lam, out, T, st); break;
    case 4: launch_fill_k<4>(a, y, rowok, lam, out, T, st); break;
    case 5: launch_fill_k<5>(a, y, rowok, lam, out, T, st); break;
    case 6: launch_fill_k<6>(a, y, rowok, lam, out, T, st); break;
    case 7: launch_fill_k<7>(a, y, rowok, lam, out, T, st); break;
    default: launch_fill_k<8>(a, y, rowok, lam, out, T, st); break;
  }
}
