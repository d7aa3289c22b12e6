// Tree-sorted portfolios (qtree.h): D nested conditional quantile splits of every period's rows on
// a tree (c_1, .., c_D) of key columns, every node of every level a portfolio, on the panel rows
// already resident in HBM.
//
//   k_qtree_port  grid (P trees, T periods), 256 threads: a workgroup handles one tree of one
//                 period. Thread tid works on the rows tid, tid + 256, ..; the keys are re-read
//                 from the panel on every sweep, never staged, so the period length is unbounded
//                 (k_qsort2_port's row access; neighbouring workgroups, x fastest, share the
//                 period's rows in L2).
//
// Keys go through the order-preserving map of qsort_dev.h (bf16 characteristics in the key's high
// half, their levels stop at bit 16; the extra keys are fp32 and take all levels). The keys of a
// tree may have different widths: each level's select runs to its own lowest bit.
//
// Level l = 1..D is one multi-set radix select, k_qsort2_port's B select with the row's set being
// its node of level l - 1: n_{l-1} sets of Q_l - 1 breakpoints, breakpoint (a, d) starts at rank
// ceil(d m_a / Q_l) - 1 of its set. An 8-bit radix level from the top, then 5-bit levels, integer
// LDS histograms, a wave prefix scan per breakpoint (qsel_wave_scan). n_{l-1} (Q_l - 1) < n_l <= 36,
// so a level has at most 35 breakpoints; n_{l-1} <= 18 sets x 256 bins at the first radix level,
// later at most 35 groups of equal prefixes x 32 bins (prefixes are non-decreasing in d within a
// set, so equal ones are adjacent; set a's groups live in the slots a (Q_l - 1) .. of the histogram).
// In a counting sweep a row finds its set by walking the breakpoint tables of the levels 1..l-1
// (LDS, sm.bk in the breaks layout): it loads its l - 1 earlier keys and its level-l key.
// At the last radix level a breakpoint's bin holds exactly the rows equal to it, so
// #{key <= b_{a,d}} within the set falls out of the scan and with it the sizes of the level-l nodes
// (no counting sweep). A node without rows has no group; its breakpoints are NaN and, as table
// entries, 0xFFFFFFFF (no row reaches it).
// A level on a bf16 key is 3 sweeps, on an fp32 key 6; then one assign sweep.
//
// Assign (k_qsort2_port's scheme, so that at D = 2 the leaf sums are its cell sums bit for bit):
// one sweep walks every row to its leaf. The rows go through LDS in chunks of 1024 (4 loads in
// flight per lane): a chunk's leaves and values are staged in row order, then thread (segment s,
// leaf c), with S = floor(256 / L) segments, adds the values of the rows of the chunk's s-th part
// that fell in leaf c to its fp64 sums, in row order; at the end the S partial sums of a leaf are
// added in segment order. Leaf counts: integer LDS atomics. Then leaves-up: an internal node's
// count is the sum of its children's counts and its fp64 sum its children's sums added in
// ascending child order. No float atomics and no scratch; the order of every sum is a function of
// n and the splits alone: repeated calls are bitwise identical.
//
// Static LDS per workgroup: histograms 18 432 B (18 sets x 256 bins x 4 B; in the assign sweep the
// staged chunk, 1024 x (1 + 3) x 4 B; after it the node sums, 72 x 3 x 8 B), partial sums
// 256 x 3 x 8 B = 6 144 B, select state, tables and node counts ~1.9 KB: ~26.5 KB of the CU's
// 160 KB, six workgroups per CU. The launch bound asks for the registers to allow six too (78 / 79
// VGPRs, no spills; without it 89 / 90 and five: measured, profiles/tree_sorts_timing.txt).
// An empty period writes its zero counts / sums and NaN breakpoints and reads no row.
#include "common.h"
#include "qtree.h"
#include "qsort_dev.h"

#define QTNT 256
#define QTMD QTREE_MAX_D
#define QTML QTREE_MAX_LEAVES
#define QTMN QTREE_MAX_NODES
#define QTMS 18                    // sets of a select: the nodes one level above a level of <= 36
#define QTMI 36                    // breakpoints of a select (<= 35), of a whole tree (L - 1 <= 35)
#define QTHW (QTMS * 256)          // histogram words
#define QTMAXV (1 + QTREE_MAX_VALUES)
#define QTUC 4                     // rows a lane loads before it processes them
#define QTCH (QTNT * QTUC)         // rows of an assign chunk: (1 + QTMAXV) * QTCH words fit the histograms

static_assert((1 + QTMAXV) * QTCH <= QTHW, "the staged chunk lives in the histograms");
static_assert(QTMN * QTMAXV * 2 <= QTHW, "the node sums live in the histograms");

struct QtSmem {
  double red[QTNT * QTMAXV];         // [segments][leaves][1 + K], segments * leaves <= 256
  uint32_t hist[QTHW];               // (8-byte aligned: the node sums are read from here)
  uint32_t pfx[QTMI], rnk[QTMI], rnk0[QTMI], cum[QTMI], gpfx[QTMI];
  int grp[QTMI];
  int ngrp[QTMS];
  uint32_t bk[QTMI];                 // the tree's breakpoints as keys, breaks layout
  int pop[QTMN];                     // rows of every node (from the selects), node layout
  int cnt[QTMN];                     // counts as written (leaves: atomics; then leaves-up)
  int Q[QTMD], key[QTMD], nn[QTMD + 1], off[QTMD + 2], boff[QTMD + 1];
};

// the tree's level-m key of compact row r
template <bool F32>
DLAP_DEV uint32_t qt_key(const QtreeArgs& a, int c, int t, int r) {
  const bool ch = c < a.pv.F;
  const float* ext = ch ? nullptr : a.extra + ((size_t)(c - a.pv.F) * a.pv.T + t) * a.pv.N;
  return qkey_load<F32>(a.pv, ch, ch ? c : 0, ext, r);
}

template <bool F32, int K1>
__global__ __launch_bounds__(QTNT, 6) void k_qtree_port(QtreeArgs a) {
  const int p = blockIdx.x, t = blockIdx.y, D = a.D;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = gp(a.pv.row_ptr)[t], n = gp(a.pv.row_ptr)[t + 1] - r0;
  int L = 1, NN = 1;
#pragma unroll
  for (int k = 0; k < QTMD; ++k)
    if (k < D) { L *= a.Q[k]; NN += L; }
  const int NB = L - 1;
  const size_t ob = (size_t)t * a.P + p;
  const float qnan = __uint_as_float(0x7FC00000u);
  if (n <= 0) {                                        // empty period: no row is read
    for (int i = tid; i < NN; i += QTNT) gp(a.count)[ob * NN + i] = 0;
    for (int i = tid; i < NN * K1; i += QTNT) gp(a.sum)[ob * NN * K1 + i] = 0.0;
    for (int i = tid; i < NB; i += QTNT) gp(a.breaks)[ob * NB + i] = qnan;
    return;
  }

  __shared__ QtSmem sm;
  if (tid == 0) {                                      // the layout of qtree.h
    int nl = 1, o = 1, bo = 0;
    sm.nn[0] = 1; sm.off[0] = 0; sm.off[1] = 1; sm.boff[0] = 0;
#pragma unroll
    for (int k = 0; k < QTMD; ++k)
      if (k < D) {
        const int q = a.Q[k];
        sm.Q[k] = q;
        sm.key[k] = gp(a.trees)[(size_t)p * D + k];
        bo += nl * (q - 1); nl *= q; o += nl;
        sm.nn[k + 1] = nl; sm.off[k + 2] = o; sm.boff[k + 1] = bo;
      }
    sm.pop[0] = n;
  }
  __syncthreads();

#pragma unroll 1
  for (int l = 1; l <= D; ++l) {                       // level l: the sets are the nodes of level l - 1
    const int Ql = sm.Q[l - 1], nb = Ql - 1, nsets = sm.nn[l - 1], ni = nsets * nb;
    const int po = sm.off[l - 1], co = sm.off[l], bo = sm.boff[l - 1];
    const int kc = sm.key[l - 1];
    const bool k16 = !F32 && kc < a.pv.F;
    const int low = k16 ? 16 : 0;                      // the key's lowest significant bit
    if (tid < ni) {
      const int s = tid / nb, d = tid - s * nb + 1;
      const int np = sm.pop[po + s];
      // ceil(d np / Ql) - 1 in [0, np) for the live breakpoints of a set with rows
      const uint32_t rk = np > 0 ? (uint32_t)(((long)d * np + Ql - 1) / Ql - 1) : 0u;
      sm.pfx[tid] = 0u; sm.rnk[tid] = rk; sm.rnk0[tid] = rk; sm.cum[tid] = 0u;
    }
    __syncthreads();

    int sh = 24, bits = 8;
#pragma unroll 1
    for (int lev = 0;; ++lev) {
      if (lev > 0 && tid < nsets) {                    // groups of equal prefixes (adjacent in d)
        int ng = 0;
        if (sm.pop[po + tid] > 0) {
          const int b = tid * nb;
          for (int d = 0; d < nb; ++d) {
            if (d == 0 || sm.pfx[b + d] != sm.pfx[b + d - 1]) sm.gpfx[b + ng++] = sm.pfx[b + d];
            sm.grp[b + d] = b + ng - 1;
          }
        }
        sm.ngrp[tid] = ng;
      }
      const int hw = lev == 0 ? nsets * 256 : ni * 32;   // <= 18 * 256, <= 35 * 32
      for (int k = tid; k < hw; k += QTNT) sm.hist[k] = 0u;
      __syncthreads();
      for (int j0 = tid; j0 < n; j0 += QTNT * QTUC) {  // QTUC independent loads in flight per lane
        uint32_t u[QTUC];
        int nd[QTUC];
#pragma unroll
        for (int k = 0; k < QTUC; ++k) {
          const int j = j0 + k * QTNT;
          u[k] = j < n ? qt_key<F32>(a, kc, t, r0 + j) : 0u;
          nd[k] = 0;
        }
#pragma unroll 1
        for (int m = 0; m < l - 1; ++m) {              // the row's node, one earlier level at a time
          const int cm = sm.key[m], Qm = sm.Q[m], bm = sm.boff[m];
          uint32_t ua[QTUC];
#pragma unroll
          for (int k = 0; k < QTUC; ++k) {
            const int j = j0 + k * QTNT;
            ua[k] = j < n ? qt_key<F32>(a, cm, t, r0 + j) : 0u;
          }
#pragma unroll
          for (int k = 0; k < QTUC; ++k) {
            const uint32_t* b = sm.bk + bm + nd[k] * (Qm - 1);   // nd < n_m: inside the level's table
            int q = 0;
            for (int d = 0; d < Qm - 1; ++d) q += ua[k] > b[d] ? 1 : 0;
            nd[k] = nd[k] * Qm + q;
          }
        }
#pragma unroll
        for (int k = 0; k < QTUC; ++k) {
          if (j0 + k * QTNT >= n) break;
          const int s = nd[k];                         // < nsets
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
      for (int k = w; k < ni; k += QTNT / 64) {
        const int s = k / nb;
        if (sm.pop[po + s] <= 0) continue;             // (the whole wave: k is the wave's)
        const uint32_t* h = sm.hist + (lev == 0 ? s * 256 : sm.grp[k] * 32);
        const uint32_t rk = sm.rnk[k];
        uint32_t dg, cb, cs;
        if (qsel_wave_scan(h, 1 << bits, rk, lane, dg, cb, cs)) {   // exactly one lane
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

    // the level's breakpoints (table and output) and the sizes of its nodes
    if (tid < ni) {
      const bool on = sm.pop[po + tid / nb] > 0;
      sm.bk[bo + tid] = on ? sm.pfx[tid] << low : 0xFFFFFFFFu;
      gp(a.breaks)[ob * NB + bo + tid] = on ? qkey_f32(sm.pfx[tid] << low, k16) : qnan;
    }
    if (tid < nsets * Ql) {
      // child q of set s holds the rows with b_{s,q} < key <= b_{s,q+1}
      const int s = tid / Ql, q = tid - s * Ql, np = sm.pop[po + s];
      const int hi = q < nb ? (int)sm.cum[s * nb + q] : np, lo = q > 0 ? (int)sm.cum[s * nb + q - 1] : 0;
      sm.pop[co + tid] = np > 0 ? hi - lo : 0;
    }
    if (l == D && tid < QTMN) sm.cnt[tid] = 0;
    __syncthreads();
  }

  // (every thread passed the barrier after the last scan: the histograms are free for the staging)
  int* rc = reinterpret_cast<int*>(sm.hist);             // [QTCH] the rows' leaves
  float* rv = reinterpret_cast<float*>(sm.hist) + QTCH;  // [K1][QTCH] the rows' values
  const int S = QTNT / L;                                // segments of a chunk, >= 7
  const int myleaf = tid % L, seg = tid / L;             // (seg >= S: the spare threads)
  const int lo = sm.off[D];                              // the first leaf's node
  double acc[K1];
#pragma unroll
  for (int v = 0; v < K1; ++v) acc[v] = 0.0;

  for (int j0 = 0; j0 < n; j0 += QTCH) {                 // chunks of QTCH rows, QTUC per lane
    float val[QTUC][K1];
    int nd[QTUC];
#pragma unroll
    for (int k = 0; k < QTUC; ++k) {
      const int j = j0 + tid + k * QTNT, r = r0 + j;
      const bool in = j < n;
      nd[k] = 0;
      val[k][0] = in ? gp(a.pv.Rc)[r] : 0.f;
      if constexpr (K1 > 1) {
        const int i = in ? gp(a.pv.rowti)[r].y : 0;
#pragma unroll
        for (int v = 1; v < K1; ++v) val[k][v] = in ? gp(a.values)[((size_t)(v - 1) * a.pv.T + t) * a.pv.N + i] : 0.f;
      }
    }
#pragma unroll 1
    for (int m = 0; m < D; ++m) {
      const int cm = sm.key[m], Qm = sm.Q[m], bm = sm.boff[m];
      uint32_t ua[QTUC];
#pragma unroll
      for (int k = 0; k < QTUC; ++k) {
        const int j = j0 + tid + k * QTNT;
        ua[k] = j < n ? qt_key<F32>(a, cm, t, r0 + j) : 0u;
      }
#pragma unroll
      for (int k = 0; k < QTUC; ++k) {
        const uint32_t* b = sm.bk + bm + nd[k] * (Qm - 1);
        int q = 0;
        for (int d = 0; d < Qm - 1; ++d) q += ua[k] > b[d] ? 1 : 0;
        nd[k] = nd[k] * Qm + q;
      }
    }
#pragma unroll
    for (int k = 0; k < QTUC; ++k) {
      const int x = tid + k * QTNT;                      // the row's place in the chunk
      if (j0 + x >= n) break;
      rc[x] = nd[k];                                     // < L
#pragma unroll
      for (int v = 0; v < K1; ++v) rv[v * QTCH + x] = val[k][v];
      atomicAdd(&sm.cnt[lo + nd[k]], 1);
    }
    __syncthreads();
    const int m = min(QTCH, n - j0), Ls = (m + S - 1) / S;  // the chunk's rows, rows per segment
    if (seg < S) {
      const int x1 = min(m, (seg + 1) * Ls);
      for (int x = seg * Ls; x < x1; ++x) {              // in row order
        const bool hit = rc[x] == myleaf;
#pragma unroll
        for (int v = 0; v < K1; ++v) acc[v] += hit ? (double)rv[v * QTCH + x] : 0.0;
      }
    }
    __syncthreads();
  }
  const int CK = L * K1;
  if (seg < S) {
#pragma unroll
    for (int v = 0; v < K1; ++v) sm.red[seg * CK + myleaf * K1 + v] = acc[v];
  }
  __syncthreads();
  // (the staged chunk is dead after the loop's last barrier: the node sums take its place)
  double* ns = reinterpret_cast<double*>(sm.hist);       // [NN][K1], node layout
  for (int i = tid; i < CK; i += QTNT) {                 // the segments in a fixed order
    double x = sm.red[i];
    for (int k = 1; k < S; ++k) x += sm.red[k * CK + i];
    ns[lo * K1 + i] = x;
  }
  __syncthreads();
#pragma unroll 1
  for (int l = D - 1; l >= 0; --l) {                     // leaves-up: the children in ascending order
    const int Qc = sm.Q[l], nl = sm.nn[l], o = sm.off[l], oc = sm.off[l + 1];
    for (int i = tid; i < nl * K1; i += QTNT) {
      const int node = i / K1, v = i - node * K1;
      const double* c = ns + (size_t)(oc + node * Qc) * K1 + v;
      double x = c[0];
      for (int q = 1; q < Qc; ++q) x += c[q * K1];
      ns[(o + node) * K1 + v] = x;
    }
    for (int i = tid; i < nl; i += QTNT) {
      int x = 0;
      for (int q = 0; q < Qc; ++q) x += sm.cnt[oc + i * Qc + q];
      sm.cnt[o + i] = x;
    }
    __syncthreads();
  }
  for (int i = tid; i < NN * K1; i += QTNT) gp(a.sum)[ob * NN * K1 + i] = ns[i];
  for (int i = tid; i < NN; i += QTNT) gp(a.count)[ob * NN + i] = sm.cnt[i];
}

template <bool F32>
static void qtree_launch_k(const QtreeArgs& a, dim3 grid, hipStream_t st) {
  switch (a.K) {
    case 0: hipLaunchKernelGGL((k_qtree_port<F32, 1>), grid, dim3(QTNT), 0, st, a); break;
    case 1: hipLaunchKernelGGL((k_qtree_port<F32, 2>), grid, dim3(QTNT), 0, st, a); break;
    default: hipLaunchKernelGGL((k_qtree_port<F32, 3>), grid, dim3(QTNT), 0, st, a); break;
  }
}

void launch_qtree_port(const QtreeArgs& a, hipStream_t st) {
  int off[QTREE_MAX_D + 2], boff[QTREE_MAX_D + 1];
  if (!qtree_layout(a.Q, a.D, off, boff) || a.K < 0 || a.K > QTREE_MAX_VALUES || a.P < 0 || a.E < 0 || a.pv.F < 0 ||
      a.pv.T > 65535 || (a.P > 0 && !a.trees) || (a.E > 0 && !a.extra) || (a.K > 0 && !a.values))
    dlap_throw_hip(hipErrorInvalidValue, "qtree_port: unsupported arguments", __FILE__, __LINE__);
  if (a.pv.T <= 0 || a.P <= 0) return;
  const dim3 grid((unsigned)a.P, (unsigned)a.pv.T);
  if (a.pv.fp32) qtree_launch_k<true>(a, grid, st);
  else qtree_launch_k<false>(a, grid, st);
  HIP_OK(hipGetLastError());
}
