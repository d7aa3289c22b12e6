// Double-sorted portfolios (qsort2.h): a Qa x Qb two-way quantile sort of every period's rows on
// a pair of key columns (A, B), on the panel rows already resident in HBM.
//
//   k_qsort2_port  grid (P pairs, T periods), 256 threads: a workgroup handles one pair of one
//                  period. Thread tid works on the rows tid, tid + 256, ..; the keys are re-read
//                  from the panel on every sweep, never staged, so the period length is unbounded.
//                  A pair's two columns are anywhere in the row, so a lane's load touches a cache
//                  line of its own (k_qsort_port's 8 adjacent columns per row are not available
//                  here); neighbouring workgroups (x fastest) share the period's rows in L2.
//
// Keys go through the order-preserving map of qsort_dev.h (bf16 characteristics in the key's high
// half, their levels stop at bit 16; the extra keys are fp32 and take all levels). The two keys
// of a pair may have different widths: each select runs to its own lowest bit.
//
// Two selects with one code path (k_qsort_port's multi-level radix select: an 8-bit level from the
// top, then 5-bit levels, integer LDS histograms, a wave prefix scan per breakpoint):
//   A   one set of Qa - 1 breakpoints over the period's n rows. At the last level a breakpoint's
//       bin holds exactly the rows equal to it, so #{A <= bA_d} = rank - residual rank + bin count
//       falls out of the scan, and with it the bucket sizes n_a (no counting sweep).
//   B   conditional: Qa sets (one per A bucket) of Qb - 1 breakpoints, breakpoint (a, d) starts at
//       rank ceil(d n_a / Qb) - 1; a sweep loads both keys of a row, finds qa from A's breakpoints
//       (LDS) and counts the row in its set. Independent: one set over all n rows, A is not read.
//   Prefixes are non-decreasing in d within a set, so equal ones are adjacent there: a set is one
//   group at the first level (256 bins) and at most Qb - 1 groups later (32 bins each); set a's
//   groups live in the slots a (Qb - 1) .. of the histogram. A set without rows (n_a = 0) has no
//   group, its breakpoints are NaN.
// bf16 pair: 3 + 3 count sweeps + the assign sweep = 7 passes; fp32 pair: 6 + 6 + 1.
//
// Assign: qa = #{d : A > bA_d} (breakpoints in registers), qb = #{d : B > bB_{qa,d}} (LDS table),
// cell = qa Qb + qb. The rows go through LDS in chunks of 1024 (4 loads in flight per lane): a
// chunk's cells and values are staged in row order, then thread (segment s, cell c), with
// S = floor(256 / (Qa Qb)) segments, adds the values of the rows of the chunk's s-th part that fell
// in cell c to its fp64 sums, in row order; at the end the S partial sums of a cell are added in
// segment order. No float atomics, and the order of every sum is a function of n alone: repeated
// calls are bitwise identical. 36 x (1 + K) register accumulators per lane (k_qsort_port's scheme)
// were measured first: 217 VGPRs at K = 1 held the kernel to 2 workgroups per CU and it ran
// 2.2 x slower (profiles/double_sorts_timing.txt). Cell counts: integer LDS atomics.
//
// Static LDS per workgroup: histograms 16 384 B (first level: Qa <= 16 sets x 256 bins x 4 B;
// later levels: <= 34 groups x 32 bins x 4 B = 4 352 B in the same space; in the assign sweep the
// staged chunk, 1024 x (1 + 3) x 4 B), partial sums 256 x 3 x 8 B = 6 144 B, breakpoint state and
// tables ~2.4 KB: ~25 KB of the CU's 160 KB, six workgroups per CU. Registers per instantiation:
// profiles/double_sorts_timing.txt.
// An empty period writes its zero counts / sums and NaN breakpoints and reads no row.
#include "common.h"
#include "qsort2.h"
#include "qsort_dev.h"

#define Q2NT 256
#define Q2MQ QSORT2_MAX_Q
#define Q2MC QSORT2_MAX_CELLS
#define Q2MI 36                    // breakpoints of a select: <= 15 (A), Qa (Qb - 1) <= 34 (B)
#define Q2HW (Q2MQ * 256)          // histogram words
#define Q2MAXV (1 + QSORT2_MAX_VALUES)
#define Q2UC 4                     // rows a lane loads before it processes them
#define Q2CH (Q2NT * Q2UC)         // rows of an assign chunk: (1 + Q2MAXV) * Q2CH words fit the histograms

struct Q2Smem {
  double red[Q2NT * Q2MAXV];         // [segments][cells][1 + K], segments * cells <= 256
  uint32_t hist[Q2HW];
  uint32_t pfx[Q2MI], rnk[Q2MI], rnk0[Q2MI], cum[Q2MI], gpfx[Q2MI];
  int grp[Q2MI];
  int ngrp[Q2MQ], npop[Q2MQ], na[Q2MQ];
  uint32_t bkA[Q2MQ], bkB[Q2MQ][Q2MQ];
  int cntl[Q2MC];
};

template <bool F32, int K1>
__global__ __launch_bounds__(Q2NT) void k_qsort2_port(Qsort2Args a) {
  const int p = blockIdx.x, t = blockIdx.y, Qa = a.Qa, Qb = a.Qb, nba = Qa - 1, nbb = Qb - 1, nc = Qa * Qb;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = gp(a.pv.row_ptr)[t], n = gp(a.pv.row_ptr)[t + 1] - r0;
  const size_t ob = (size_t)t * a.P + p;
  const float qnan = __uint_as_float(0x7FC00000u);
  if (n <= 0) {                                        // empty period: no row is read
    for (int i = tid; i < nc; i += Q2NT) gp(a.count)[ob * nc + i] = 0;
    for (int i = tid; i < nc * K1; i += Q2NT) gp(a.sum)[ob * nc * K1 + i] = 0.0;
    for (int i = tid; i < nba; i += Q2NT) gp(a.breaks_a)[ob * nba + i] = qnan;
    for (int i = tid; i < Qa * nbb; i += Q2NT) gp(a.breaks_b)[ob * Qa * nbb + i] = qnan;
    return;
  }
  const int2 pr = gp(a.pairs)[p];
  const bool charA = pr.x < a.pv.F, charB = pr.y < a.pv.F;
  const int colA = charA ? pr.x : 0, colB = charB ? pr.y : 0;
  const float* extA = charA ? nullptr : a.extra + ((size_t)(pr.x - a.pv.F) * a.pv.T + t) * a.pv.N;
  const float* extB = charB ? nullptr : a.extra + ((size_t)(pr.y - a.pv.F) * a.pv.T + t) * a.pv.N;
  const bool k16A = !F32 && charA, k16B = !F32 && charB;
  const int lowA = k16A ? 16 : 0, lowB = k16B ? 16 : 0;   // the keys' lowest significant bits
  const bool cond = a.conditional != 0;

  __shared__ Q2Smem sm;

#pragma unroll 1
  for (int ph = 0; ph < 2; ++ph) {                     // select A, then B
    const bool cnd = ph == 1 && cond;                  // the row's set is its A bucket
    const int nsets = cnd ? Qa : 1, nb = ph == 0 ? nba : nbb, Qx = ph == 0 ? Qa : Qb, ni = nsets * nb;
    const bool kchar = ph == 0 ? charA : charB;
    const int kcol = ph == 0 ? colA : colB, low = ph == 0 ? lowA : lowB;
    const float* kext = ph == 0 ? extA : extB;
    if (tid < Q2MQ) sm.npop[tid] = tid >= nsets ? 0 : (cnd ? sm.na[tid] : n);
    if (tid < ni) {
      const int s = tid / nb, d = tid - s * nb + 1;
      const int np = cnd ? sm.na[s] : n;
      // ceil(d np / Qx) - 1 in [0, np) for the live breakpoints of a set with rows
      const uint32_t rk = np > 0 ? (uint32_t)(((long)d * np + Qx - 1) / Qx - 1) : 0u;
      sm.pfx[tid] = 0u; sm.rnk[tid] = rk; sm.rnk0[tid] = rk; sm.cum[tid] = 0u;
    }
    __syncthreads();

    int sh = 24, bits = 8;
#pragma unroll 1
    for (int lev = 0;; ++lev) {
      if (lev > 0 && tid < nsets) {                    // groups of equal prefixes (adjacent in d)
        int ng = 0;
        if (sm.npop[tid] > 0) {
          const int b = tid * nb;
          for (int d = 0; d < nb; ++d) {
            if (d == 0 || sm.pfx[b + d] != sm.pfx[b + d - 1]) sm.gpfx[b + ng++] = sm.pfx[b + d];
            sm.grp[b + d] = b + ng - 1;
          }
        }
        sm.ngrp[tid] = ng;
      }
      const int hw = lev == 0 ? nsets * 256 : ni * 32;   // <= 16 * 256, <= 34 * 32
      for (int k = tid; k < hw; k += Q2NT) sm.hist[k] = 0u;
      __syncthreads();
      for (int j0 = tid; j0 < n; j0 += Q2NT * Q2UC) {  // Q2UC independent loads in flight per lane
        uint32_t u[Q2UC], ua[Q2UC];
#pragma unroll
        for (int k = 0; k < Q2UC; ++k) {
          const int j = j0 + k * Q2NT;
          u[k] = j < n ? qkey_load<F32>(a.pv, kchar, kcol, kext, r0 + j) : 0u;
          ua[k] = cnd && j < n ? qkey_load<F32>(a.pv, charA, colA, extA, r0 + j) : 0u;
        }
#pragma unroll
        for (int k = 0; k < Q2UC; ++k) {
          if (j0 + k * Q2NT >= n) break;
          int s = 0;
          if (cnd)
            for (int d = 0; d < nba; ++d) s += ua[k] > sm.bkA[d] ? 1 : 0;
          const uint32_t dg = (u[k] >> sh) & ((1u << bits) - 1u);
          if (lev == 0) atomicAdd(&sm.hist[s * 256 + dg], 1u);
          else {
            const uint32_t hi = u[k] >> (sh + bits);
            const int b = s * nb, ng = sm.ngrp[s];
            for (int g = 0; g < ng; ++g)
              if (sm.gpfx[b + g] == hi) { atomicAdd(&sm.hist[(b + g) * 32 + dg], 1u); break; }
          }
        }
      }
      __syncthreads();
      // breakpoint: the bin of its group's histogram that holds residual rank rnk
      const int nbins = 1 << bits;
      for (int k = w; k < ni; k += Q2NT / 64) {
        const int s = k / nb;
        if (sm.npop[s] <= 0) continue;                 // (the whole wave: k is the wave's)
        const uint32_t* h = sm.hist + (lev == 0 ? s * 256 : sm.grp[k] * 32);
        const uint32_t rk = sm.rnk[k];
        const int b0 = 4 * lane;
        const uint32_t c0 = b0 < nbins ? h[b0] : 0u, c1 = b0 + 1 < nbins ? h[b0 + 1] : 0u;
        const uint32_t c2 = b0 + 2 < nbins ? h[b0 + 2] : 0u, c3 = b0 + 3 < nbins ? h[b0 + 3] : 0u;
        const uint32_t sb = c0 + c1 + c2 + c3;
        uint32_t inc = sb;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t v = __shfl_up(inc, o, 64);
          if (lane >= o) inc += v;
        }
        uint32_t cb = inc - sb;                        // rows in the bins below this lane's
        if (cb <= rk && rk < inc) {                    // exactly one lane: rk < the group's rows
          uint32_t dg = (uint32_t)b0, cs = c0;
          if (rk >= cb + c0) { cb += c0; ++dg; cs = c1;
            if (rk >= cb + c1) { cb += c1; ++dg; cs = c2;
              if (rk >= cb + c2) { cb += c2; ++dg; cs = c3; } } }
          sm.pfx[k] = (sm.pfx[k] << bits) | dg;
          sm.rnk[k] = rk - cb;
          // rows below the bin + rows in it; at the last level the bin is the breakpoint's value,
          // so this is #{key <= breakpoint} within the set
          sm.cum[k] = sm.rnk0[k] - (rk - cb) + cs;
        }
      }
      __syncthreads();
      if (sh == low) break;
      bits = min(5, sh - low);
      sh -= bits;
    }

    if (ph == 0) {
      if (tid < Q2MQ) {
        sm.bkA[tid] = tid < nba ? sm.pfx[tid] << lowA : 0xFFFFFFFFu;
        // bucket a holds the rows with bA_a < A <= bA_{a+1}
        const int hi = tid < nba ? (int)sm.cum[tid] : n, lo = tid > 0 && tid <= nba ? (int)sm.cum[tid - 1] : 0;
        sm.na[tid] = tid < Qa ? hi - lo : 0;
      }
      for (int i = tid; i < nba; i += Q2NT) gp(a.breaks_a)[ob * nba + i] = qkey_f32(sm.pfx[i] << lowA, k16A);
      __syncthreads();
    }
  }

  // B's breakpoint table (independent mode: one set for every a) and the breaks_b output
  {
    const int s = tid / Q2MQ, d = tid % Q2MQ, src = cond ? s : 0;
    const bool on = s < Qa && d < nbb && sm.npop[src] > 0;
    (&sm.bkB[0][0])[tid] = on ? sm.pfx[src * nbb + d] << lowB : 0xFFFFFFFFu;
    if (s < Qa && d < nbb)
      gp(a.breaks_b)[(ob * Qa + s) * nbb + d] = on ? qkey_f32(sm.pfx[src * nbb + d] << lowB, k16B) : qnan;
    if (tid < Q2MC) sm.cntl[tid] = 0;
  }
  uint32_t bk[Q2MQ - 1];
#pragma unroll
  for (int d = 0; d < Q2MQ - 1; ++d) bk[d] = sm.bkA[d];  // (the unused slots hold 0xFFFFFFFF)
  __syncthreads();

  // (every thread passed the barrier after the last scan: the histograms are free for the staging)
  int* rc = reinterpret_cast<int*>(sm.hist);             // [Q2CH] the rows' cells
  float* rv = reinterpret_cast<float*>(sm.hist) + Q2CH;  // [K1][Q2CH] the rows' values
  const int S = Q2NT / nc;                               // segments of a chunk, >= 7
  const int mycell = tid % nc, seg = tid / nc;           // (seg >= S: the spare threads)
  double acc[K1];
#pragma unroll
  for (int v = 0; v < K1; ++v) acc[v] = 0.0;

  for (int j0 = 0; j0 < n; j0 += Q2CH) {                 // chunks of Q2CH rows, Q2UC per lane
    uint32_t ua[Q2UC], ub[Q2UC];
    float val[Q2UC][K1];
#pragma unroll
    for (int k = 0; k < Q2UC; ++k) {
      const int j = j0 + tid + k * Q2NT, r = r0 + j;
      const bool in = j < n;
      ua[k] = in ? qkey_load<F32>(a.pv, charA, colA, extA, r) : 0u;
      ub[k] = in ? qkey_load<F32>(a.pv, charB, colB, extB, r) : 0u;
      val[k][0] = in ? gp(a.pv.Rc)[r] : 0.f;
      if constexpr (K1 > 1) {
        const int i = in ? gp(a.pv.rowti)[r].y : 0;
#pragma unroll
        for (int v = 1; v < K1; ++v) val[k][v] = in ? gp(a.values)[((size_t)(v - 1) * a.pv.T + t) * a.pv.N + i] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < Q2UC; ++k) {
      const int x = tid + k * Q2NT;                      // the row's place in the chunk
      if (j0 + x >= n) break;
      int qa = 0, qb = 0;
#pragma unroll
      for (int d = 0; d < Q2MQ - 1; ++d) qa += ua[k] > bk[d] ? 1 : 0;
      for (int d = 0; d < nbb; ++d) qb += ub[k] > sm.bkB[qa][d] ? 1 : 0;
      const int cell = qa * Qb + qb;                     // qa < Qa, qb < Qb: cell < nc
      rc[x] = cell;
#pragma unroll
      for (int v = 0; v < K1; ++v) rv[v * Q2CH + x] = val[k][v];
      atomicAdd(&sm.cntl[cell], 1);
    }
    __syncthreads();
    const int m = min(Q2CH, n - j0), L = (m + S - 1) / S;  // the chunk's rows, rows per segment
    if (seg < S) {
      const int x1 = min(m, (seg + 1) * L);
      for (int x = seg * L; x < x1; ++x) {               // in row order
        const bool hit = rc[x] == mycell;
#pragma unroll
        for (int v = 0; v < K1; ++v) acc[v] += hit ? (double)rv[v * Q2CH + x] : 0.0;
      }
    }
    __syncthreads();
  }
  const int CK = nc * K1;
  if (seg < S) {
#pragma unroll
    for (int v = 0; v < K1; ++v) sm.red[seg * CK + mycell * K1 + v] = acc[v];
  }
  __syncthreads();
  for (int i = tid; i < CK; i += Q2NT) {                 // the segments in a fixed order
    double x = sm.red[i];
    for (int k = 1; k < S; ++k) x += sm.red[k * CK + i];
    gp(a.sum)[ob * CK + i] = x;
  }
  for (int i = tid; i < nc; i += Q2NT) gp(a.count)[ob * nc + i] = sm.cntl[i];
}

template <bool F32>
static void qsort2_launch_k(const Qsort2Args& a, dim3 grid, hipStream_t st) {
  switch (a.K) {
    case 0: hipLaunchKernelGGL((k_qsort2_port<F32, 1>), grid, dim3(Q2NT), 0, st, a); break;
    case 1: hipLaunchKernelGGL((k_qsort2_port<F32, 2>), grid, dim3(Q2NT), 0, st, a); break;
    default: hipLaunchKernelGGL((k_qsort2_port<F32, 3>), grid, dim3(Q2NT), 0, st, a); break;
  }
}

void launch_qsort2_port(const Qsort2Args& a, hipStream_t st) {
  if (a.Qa < 2 || a.Qa > QSORT2_MAX_Q || a.Qb < 2 || a.Qb > QSORT2_MAX_Q || a.Qa * a.Qb > QSORT2_MAX_CELLS ||
      a.K < 0 || a.K > QSORT2_MAX_VALUES || a.P < 0 || a.E < 0 || a.pv.F < 0 || a.pv.T > 65535 ||
      (a.P > 0 && !a.pairs) || (a.E > 0 && !a.extra) || (a.K > 0 && !a.values))
    dlap_throw_hip(hipErrorInvalidValue, "qsort2_port: unsupported arguments", __FILE__, __LINE__);
  if (a.pv.T <= 0 || a.P <= 0) return;
  const dim3 grid((unsigned)a.P, (unsigned)a.pv.T);
  if (a.pv.fp32) qsort2_launch_k<true>(a, grid, st);
  else qsort2_launch_k<false>(a, grid, st);
  HIP_OK(hipGetLastError());
}
