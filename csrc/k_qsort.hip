// Characteristic-sorted portfolios (qsort.h): quantile breakpoints by an exact multi-level radix
// select over the panel rows already resident in HBM, then one sweep that buckets every row and
// accumulates the bucket sums.
//
//   k_qsort_port  grid (key blocks, T periods), 256 threads: a workgroup handles a block of 8
//                 adjacent key columns of one period. Thread tid works on column tid & 7 of the rows
//                 tid >> 3, + 32, ..: the 8 lanes of a row read 16 contiguous bytes of its bf16 panel
//                 row (32 of an fp32 one), so a wave load touches 8 cache lines instead of the 64 a
//                 column per workgroup would, and the period's rows go through L2 once per 8
//                 columns and sweep. Neighbouring workgroups (x fastest) share the period. The keys
//                 are re-read on every sweep, never staged, so the period length is unbounded
//                 (30 000 rows on the scaled panel). The caller's extra keys come after the
//                 characteristics in blocks of their own (lane column = array, gathered by stock).
//
// Keys go through the order-preserving float -> uint32 map (sign bit flipped for positive values,
// all bits for negative ones) with -0.0 folded onto +0.0. bf16 characteristics take the same map on
// their 16 bits and sit in the key's high half: the low half is zero, so their levels stop at bit
// 16 (the extra keys are fp32 in either precision and take all levels).
//
// Select, per column: an 8-bit level from the top, then 5-bit levels (8+5+3 bits = 3 sweeps for
// bf16 keys, 8+5+5+5+5+4 = 6 for fp32 keys). Breakpoint d carries the key prefix found so far and
// its residual rank among the rows matching that prefix. Prefixes are non-decreasing in d, so equal
// ones are adjacent: they form one group at the first level (256 bins) and at most Q - 1 <= 15
// groups later (32 bins each). A sweep counts every row whose high bits match a live group
// (integer LDS atomics: integer sums do not depend on the order); then each (column, breakpoint)
// finds its digit with a wave prefix scan of its group's histogram (lane l owns bins 4l .. 4l+3).
//
// Assign: bucket = #{d : key > b_d}. A lane keeps 16 x (1 + K) fp64 sums of its column's rows in
// registers (compile-time indices: the row's value is added to its bucket's slot and +0.0 to the
// others); the 8 lanes of a column in a wave are combined by a fixed xor-shuffle tree and the four
// wave totals summed in a fixed order through LDS. No float atomics: repeated calls are bitwise
// identical.
//
// Static LDS: one 20 480 B buffer holding the histograms (8 columns x 15 groups x 32 bins x 4 B =
// 15 360 B; the first level's 8 x 256 bins fit the same space) and afterwards the wave totals
// (4 waves x 8 columns x 16 x 5 x 8 B), + 2.5 KB of breakpoint state and bucket counts = 23 KB of
// the CU's 160 KB: seven workgroups per CU fit.
// An empty period writes its zero counts / sums and NaN breakpoints and reads no row.
#include "common.h"
#include "qsort.h"
#include "qsort_dev.h"             // qkey_u32, qkey_f32, qkey_load

#define QNT 256
#define QNB (QSORT_MAX_Q - 1)
#define QCB 8                      // key columns per workgroup
#define QRS (QNT / QCB)            // rows per workgroup step
#define QHC (QNB * 32)             // histogram words per column (>= the first level's 256)
#define QMAXV (1 + QSORT_MAX_VALUES)
#define QUC 8                      // rows a lane loads before it processes them: count sweeps,
#define QUA 4                      // assign sweep (one load latency per batch instead of per row)

template <bool F32, int K1>
__global__ __launch_bounds__(QNT) void k_qsort_port(QsortArgs a) {
  const int t = blockIdx.y, NK = a.C + a.E, Q = a.Q, nb = Q - 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = tid & (QCB - 1), slot = tid >> 3;
  const int cblocks = (a.C + QCB - 1) / QCB;
  const bool is_char = (int)blockIdx.x < cblocks;
  // first key of the block and the number of its live columns
  const int k0 = is_char ? (int)blockIdx.x * QCB : a.C + ((int)blockIdx.x - cblocks) * QCB;
  const int nc = min(QCB, (is_char ? a.C : NK) - k0);
  const int r0 = gp(a.pv.row_ptr)[t], n = gp(a.pv.row_ptr)[t + 1] - r0;
  const size_t ob = (size_t)t * NK + k0;               // outputs of the block's columns are adjacent
  if (n <= 0) {                                        // empty period: no row is read
    for (int i = tid; i < nc * Q; i += QNT) gp(a.count)[ob * Q + i] = 0;
    for (int i = tid; i < nc * Q * K1; i += QNT) gp(a.sum)[ob * Q * K1 + i] = 0.0;
    for (int i = tid; i < nc * nb; i += QNT) gp(a.breaks)[ob * nb + i] = __uint_as_float(0x7FC00000u);
    return;
  }
  const bool live = c < nc;
  const int col = is_char && live ? (a.cols ? gp(a.cols)[k0 + c] : k0 + c) : 0;
  const float* ext = !is_char && live ? a.extra + ((size_t)(k0 + c - a.C) * a.pv.T + t) * a.pv.N : nullptr;

  __shared__ double red[QNT / 64 * QCB * QSORT_MAX_Q * QMAXV];     // 20 480 B, first the histograms
  uint32_t* hist = reinterpret_cast<uint32_t*>(red);               // [QCB][QHC]
  __shared__ uint32_t pfx[QCB][QNB], rnk[QCB][QNB], gpfx[QCB][QNB];
  __shared__ int grp[QCB][QNB], ngrp[QCB], cntl[QCB][QSORT_MAX_Q];

  if (tid < QCB * QSORT_MAX_Q) (&cntl[0][0])[tid] = 0;
  if (tid < QCB * QNB) {
    const int d = tid % QNB + 1;
    (&pfx[0][0])[tid] = 0u;
    // ceil(d n / Q) - 1 in [0, n) for the live breakpoints d < Q
    (&rnk[0][0])[tid] = d < Q ? (uint32_t)(((long)d * n + Q - 1) / Q - 1) : 0u;
  }
  __syncthreads();

  const bool k16 = !F32 && is_char;
  const int low = k16 ? 16 : 0;                        // the keys' lowest significant bit
  int sh = 24, bits = 8;
#pragma unroll 1
  for (int lev = 0;; ++lev) {
    if (tid < nc) {                                    // groups of equal prefixes (adjacent in d)
      int ng = 0;
      for (int d = 0; d < nb; ++d) {
        if (d == 0 || pfx[tid][d] != pfx[tid][d - 1]) gpfx[tid][ng++] = pfx[tid][d];
        grp[tid][d] = ng - 1;
      }
      ngrp[tid] = ng;
    }
    for (int k = tid; k < QCB * QHC; k += QNT) hist[k] = 0u;
    __syncthreads();
    const int gstride = lev == 0 ? 0 : 32;             // (one group of 256 bins at the first level)
    if (live) {
      const int ng = ngrp[c];
      uint32_t* hc = hist + c * QHC;
      for (int j0 = slot; j0 < n; j0 += QRS * QUC) {   // QUC independent loads in flight per lane
        uint32_t u[QUC];
#pragma unroll
        for (int k = 0; k < QUC; ++k) {
          const int j = j0 + k * QRS;
          u[k] = j < n ? qkey_load<F32>(a.pv, is_char, col, ext, r0 + j) : 0u;
        }
#pragma unroll
        for (int k = 0; k < QUC; ++k) {
          if (j0 + k * QRS >= n) break;
          const uint32_t hi = lev == 0 ? 0u : u[k] >> (sh + bits);
          const uint32_t dg = (u[k] >> sh) & ((1u << bits) - 1u);
          for (int g = 0; g < ng; ++g)
            if (gpfx[c][g] == hi) { atomicAdd(&hc[g * gstride + dg], 1u); break; }
        }
      }
    }
    __syncthreads();
    // (column, breakpoint): the bin of its group's histogram that holds residual rank rnk
    const int nbins = 1 << bits;
    for (int k = w; k < nc * nb; k += QNT / 64) {
      const int kc = k / nb, d = k - kc * nb;
      const uint32_t* h = hist + kc * QHC + grp[kc][d] * gstride;
      const uint32_t rk = rnk[kc][d];
      const int b0 = 4 * lane;
      const uint32_t c0 = b0 < nbins ? h[b0] : 0u, c1 = b0 + 1 < nbins ? h[b0 + 1] : 0u;
      const uint32_t c2 = b0 + 2 < nbins ? h[b0 + 2] : 0u, c3 = b0 + 3 < nbins ? h[b0 + 3] : 0u;
      const uint32_t s = c0 + c1 + c2 + c3;
      uint32_t inc = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      uint32_t cb = inc - s;                           // rows in the bins below this lane's
      if (cb <= rk && rk < inc) {                      // exactly one lane: rk < the group's rows
        uint32_t dg = (uint32_t)b0;
        if (rk >= cb + c0) { cb += c0; ++dg;
          if (rk >= cb + c1) { cb += c1; ++dg;
            if (rk >= cb + c2) { cb += c2; ++dg; } } }
        pfx[kc][d] = (pfx[kc][d] << bits) | dg;
        rnk[kc][d] = rk - cb;
      }
    }
    __syncthreads();
    if (sh == low) break;
    bits = min(5, sh - low);
    sh -= bits;
  }

  uint32_t bk[QNB];
#pragma unroll
  for (int d = 0; d < QNB; ++d) bk[d] = d < nb ? pfx[c][d] << low : 0xFFFFFFFFu;

  double acc[QSORT_MAX_Q][K1];
#pragma unroll
  for (int q = 0; q < QSORT_MAX_Q; ++q)
#pragma unroll
    for (int v = 0; v < K1; ++v) acc[q][v] = 0.0;

  if (live) {
    for (int j0 = slot; j0 < n; j0 += QRS * QUA) {      // (rows in increasing order, as unbatched)
      uint32_t u[QUA];
      float val[QUA][K1];
#pragma unroll
      for (int k = 0; k < QUA; ++k) {
        const int j = j0 + k * QRS, r = r0 + j;
        const bool in = j < n;
        u[k] = in ? qkey_load<F32>(a.pv, is_char, col, ext, r) : 0u;
        val[k][0] = in ? gp(a.pv.Rc)[r] : 0.f;
        if constexpr (K1 > 1) {
          const int i = in ? gp(a.pv.rowti)[r].y : 0;
#pragma unroll
          for (int v = 1; v < K1; ++v) val[k][v] = in ? gp(a.values)[((size_t)(v - 1) * a.pv.T + t) * a.pv.N + i] : 0.f;
        }
      }
#pragma unroll
      for (int k = 0; k < QUA; ++k) {
        if (j0 + k * QRS >= n) break;
        int b = 0;
#pragma unroll
        for (int d = 0; d < QNB; ++d) b += u[k] > bk[d] ? 1 : 0;   // (the unused slots hold 0xFFFFFFFF)
#pragma unroll
        for (int q = 0; q < QSORT_MAX_Q; ++q)
#pragma unroll
          for (int v = 0; v < K1; ++v) acc[q][v] += b == q ? (double)val[k][v] : 0.0;
        atomicAdd(&cntl[c][b], 1);
      }
    }
  }
  // (every thread passed the barrier after the last scan: the histograms are free for the totals)
  const int QK = Q * K1;
#pragma unroll
  for (int q = 0; q < QSORT_MAX_Q; ++q) {
    if (q < Q) {
#pragma unroll
      for (int v = 0; v < K1; ++v) {
        double x = acc[q][v];
#pragma unroll
        for (int o = 32; o >= QCB; o >>= 1) x += __shfl_xor(x, o, 64);   // the lanes of column c
        if (lane < QCB) red[(w * QCB + c) * QK + q * K1 + v] = x;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < nc * QK; i += QNT) {           // i = column * QK + (q, v)
    const int kc = i / QK, e = i - kc * QK;
    double x = red[kc * QK + e];
#pragma unroll
    for (int k = 1; k < QNT / 64; ++k) x += red[(k * QCB + kc) * QK + e];
    gp(a.sum)[ob * QK + i] = x;
  }
  for (int i = tid; i < nc * Q; i += QNT) gp(a.count)[ob * Q + i] = cntl[i / Q][i % Q];
  for (int i = tid; i < nc * nb; i += QNT)
    gp(a.breaks)[ob * nb + i] = qkey_f32(pfx[i / nb][i % nb] << low, k16);
}

template <bool F32>
static void qsort_launch_k(const QsortArgs& a, dim3 grid, hipStream_t st) {
  switch (a.K) {
    case 0: hipLaunchKernelGGL((k_qsort_port<F32, 1>), grid, dim3(QNT), 0, st, a); break;
    case 1: hipLaunchKernelGGL((k_qsort_port<F32, 2>), grid, dim3(QNT), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_qsort_port<F32, 3>), grid, dim3(QNT), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_qsort_port<F32, 4>), grid, dim3(QNT), 0, st, a); break;
    default: hipLaunchKernelGGL((k_qsort_port<F32, 5>), grid, dim3(QNT), 0, st, a); break;
  }
}

void launch_qsort_port(const QsortArgs& a, hipStream_t st) {
  if (a.Q < 2 || a.Q > QSORT_MAX_Q || a.K < 0 || a.K > QSORT_MAX_VALUES || a.C < 0 || a.E < 0 || a.pv.T > 65535 ||
      (a.E > 0 && !a.extra) || (a.K > 0 && !a.values))
    dlap_throw_hip(hipErrorInvalidValue, "qsort_port: unsupported arguments", __FILE__, __LINE__);
  if (a.pv.T <= 0 || a.C + a.E <= 0) return;
  const dim3 grid((unsigned)((a.C + QCB - 1) / QCB + (a.E + QCB - 1) / QCB), (unsigned)a.pv.T);
  if (a.pv.fp32) qsort_launch_k<true>(a, grid, st);
  else qsort_launch_k<false>(a, grid, st);
  HIP_OK(hipGetLastError());
}
