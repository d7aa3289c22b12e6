// Stock-level weights of a combination of tree nodes (qtree_weight.h) on the panel rows already
// resident in HBM.
//
//   k_qtree_weight  grid (segments), QTREE_WEIGHT_SEG threads: a workgroup handles one period's
//                   segment of QTREE_WEIGHT_SEG rows, one lane per row. The U distinct key columns
//                   of the call are staged once as order-preserving uint32 keys [U][rows] in LDS;
//                   then the active trees go through LDS in passes of tpp trees: their breakpoints
//                   as uint32 keys (NaN -> 0xFFFFFFFF, no key is above it), the fp64 table
//                   coef / count of this period (0.0 where coef == 0) and their key slots. A tree
//                   step is one key read, Q_l - 1 breakpoint reads and one table read, all LDS.
//
// Keys: qkey_row (qsort_dev.h), qkey_u32 of the fp32 value, a bf16 characteristic widened exactly first. For
// the breakpoints of a sort of the same keys that is k_qtree_port's comparison (its bf16 key is the
// same map with the low half cleared on both sides); for any other breakpoint it is still the
// float comparison of the definition.
//
// Order: a lane's acc stays in a register across the passes and takes its additions in the
// definition's order (tree ascending, level ascending). Two trees are walked side by side for the
// LDS latency, their table entries are added one tree after the other. Levels below a tree's
// deepest active one add +0.0, which changes no bit (acc is never -0.0). So no output bit depends
// on tpp, the segment size or the grid. The file is compiled with -ffp-contract=off; the acc chain
// holds divisions and additions only.
//
// No atomics, no scratch (the level loop is unrolled over the template's depth, every array index
// is static), no cross-workgroup wait, no device memory of its own. All LDS is dynamic, every
// carve offset a multiple of 16: at the default 16 trees a pass and depth 4 on 3 keys 8.4 KB.
//
// -DQTREE_WEIGHT_REREAD=1 builds the measured alternative that stages no keys and reads a level's key
// from the panel at every tree step (profiles/tree_weights_timing.txt); the LDS slots then hold the
// key columns themselves. Same bits.
#include <cmath>
#include "common.h"
#include "qtree_weight.h"
#include "qsort_dev.h"

#define QWNT QTREE_WEIGHT_SEG
#define QWMD QTREE_MAX_D
#define QWMW QTREE_WEIGHT_META
#ifndef QTREE_WEIGHT_REREAD
#define QTREE_WEIGHT_REREAD 0
#endif

static_assert(QWNT % 64 == 0 && QWNT >= 64 && QWNT <= 1024, "a segment is a whole number of waves");

struct QwCarve { unsigned cc, keys, bk, meta, total; };   // byte offsets into the dynamic LDS

DLAP_HD QwCarve qw_carve(int tpp, int NN, int NB, int U) {
  QwCarve c;
  c.cc = 0u;
  c.keys = (unsigned)(tpp * NN * 8 + 15) & ~15u;
  c.bk = c.keys + (unsigned)(U > 0 ? U : 1) * QWNT * 4u;   // (a dead level reads slot 0, also when U == 0)
  c.meta = c.bk + ((unsigned)(tpp * (NB > 0 ? NB : 1) * 4 + 15) & ~15u);
  c.total = c.meta + ((unsigned)(tpp * QWMW * 4 + 15) & ~15u);
  return c;
}

template <bool F32, int D>
__global__ __launch_bounds__(QWNT) void k_qtree_weight(QtreeWeightArgs a) {
  extern __shared__ __attribute__((aligned(16))) char qw_smem[];
  const int tid = threadIdx.x;
  const int2 sg = gp(a.seg)[blockIdx.x];
  const int t = sg.x;
  const int r0 = gp(a.pv.row_ptr)[t], n = gp(a.pv.row_ptr)[t + 1] - r0;
  const int j = sg.y + tid;
  const bool in = j < n;                                  // (the segment's first row is one: sg.y < n)
  const int r = r0 + (in ? j : sg.y);
  const int i = gp(a.pv.rowti)[r].y;                      // < N

  // the layout of qtree.h (uniform, in scalar registers after the unroll)
  int Q[D], off[D + 2], boff[D + 1];
  off[0] = 0; off[1] = 1; boff[0] = 0;
  {
    int nl = 1;
#pragma unroll
    for (int l = 1; l <= D; ++l) {
      Q[l - 1] = a.Q[l - 1];
      boff[l] = boff[l - 1] + nl * (Q[l - 1] - 1);
      nl *= Q[l - 1];
      off[l + 1] = off[l] + nl;
    }
  }
  const int NN = off[D + 1], NB = boff[D], NBp = NB > 0 ? NB : 1;
  const int tpp = a.tpp, U = a.U, P = a.P;
  const QwCarve cv = qw_carve(tpp, NN, NB, U);
  double* cc = reinterpret_cast<double*>(qw_smem + cv.cc);          // [tpp][NN]
  uint32_t* keys = reinterpret_cast<uint32_t*>(qw_smem + cv.keys);  // [U][QWNT]
  uint32_t* bk = reinterpret_cast<uint32_t*>(qw_smem + cv.bk);      // [tpp][NBp]
  int* meta = reinterpret_cast<int*>(qw_smem + cv.meta);            // [tpp][QWMW]

  // the row's key in column c of the call (c < F + E); rows beyond the segment's end carry key 0
  auto load_key = [&](int c) -> uint32_t { return in ? qkey_row<F32>(a.pv, c, a.extra, t, r, i) : 0u; };
#if QTREE_WEIGHT_REREAD
  if (tid < (U > 0 ? U : 1)) keys[tid] = U > 0 ? (uint32_t)gp(a.ucols)[tid] : 0u;   // slot -> key column (U <= 32 < threads)
#define QW_KEY(slot) load_key((int)keys[slot])
#else
  for (int u = 0; u < U; ++u) keys[u * QWNT + tid] = load_key(gp(a.ucols)[u]);   // once per segment
#define QW_KEY(slot) keys[(slot) * QWNT + tid]
#endif

  double acc = 0.0;
#pragma unroll 1
  for (int p0 = 0; p0 < a.Pa; p0 += tpp) {
    const int np = min(tpp, a.Pa - p0);
    __syncthreads();                                      // the walk of the pass before is over
    for (int x = tid; x < np * QWMW; x += QWNT) meta[x] = gp(a.meta)[(size_t)p0 * QWMW + x];
    for (int x = tid; x < np * NN; x += QWNT) {
      const int k = x / NN, jn = x - k * NN;
      const int pid = gp(a.meta)[(size_t)(p0 + k) * QWMW];                 // < P
      const double c = gp(a.coef)[(size_t)pid * NN + jn];
      const int m = gp(a.count)[((size_t)t * P + pid) * NN + jn];
      cc[x] = c != 0.0 ? c / (double)m : 0.0;                              // (-0.0 is 0)
    }
    for (int x = tid; x < np * NB; x += QWNT) {
      const int k = x / NB, jb = x - k * NB;
      const int pid = gp(a.meta)[(size_t)(p0 + k) * QWMW];
      const float b = gp(a.breaks)[((size_t)t * P + pid) * NB + jb];
      bk[k * NBp + jb] = b != b ? 0xFFFFFFFFu : qkey_u32(b);
    }
    __syncthreads();

#pragma unroll 1
    for (int k0 = 0; k0 < np; k0 += 2) {                  // two trees side by side
      const bool two = k0 + 1 < np;
      const int k1 = two ? k0 + 1 : k0;
      const int* m0 = meta + k0 * QWMW;
      const int* m1 = meta + k1 * QWMW;
      const int d0 = m0[1], d1 = two ? m1[1] : -1;        // deepest active level; -1: no tree
      const double* c0 = cc + k0 * NN;
      const double* c1 = cc + k1 * NN;
      const uint32_t* b0 = bk + k0 * NBp;
      const uint32_t* b1 = bk + k1 * NBp;
      double v0[D + 1], v1[D + 1];
      v0[0] = c0[0];
      v1[0] = two ? c1[0] : 0.0;
      int n0 = 0, n1 = 0;
#pragma unroll
      for (int l = 1; l <= D; ++l) {
        // a level below the tree's depth walks node 0 on slot 0 (inside the tables) and adds 0.0
        const bool l0 = l <= d0, l1 = l <= d1;
        const int Ql = Q[l - 1];
        const uint32_t u0 = QW_KEY(l0 ? m0[1 + l] : 0);
        const uint32_t u1 = QW_KEY(l1 ? m1[1 + l] : 0);
        const uint32_t* e0 = b0 + boff[l - 1] + (l0 ? n0 : 0) * (Ql - 1);   // n < n_{l-1}: inside the level's table
        const uint32_t* e1 = b1 + boff[l - 1] + (l1 ? n1 : 0) * (Ql - 1);
        int q0 = 0, q1 = 0;
        for (int d = 0; d < Ql - 1; ++d) {
          q0 += u0 > e0[d] ? 1 : 0;
          q1 += u1 > e1[d] ? 1 : 0;
        }
        n0 = l0 ? n0 * Ql + q0 : 0;                        // < n_l
        n1 = l1 ? n1 * Ql + q1 : 0;
        const double x0 = c0[off[l] + n0], x1 = c1[off[l] + n1];
        v0[l] = l0 ? x0 : 0.0;
        v1[l] = l1 ? x1 : 0.0;
      }
#pragma unroll
      for (int l = 0; l <= D; ++l) acc = acc + v0[l];
#pragma unroll
      for (int l = 0; l <= D; ++l) acc = acc + v1[l];
    }
  }
  if (in) {
    const size_t o = (size_t)t * a.pv.N + i;
    gp(a.w_out)[o] = (float)acc;
    if (a.acc_out) gp(a.acc_out)[o] = acc;
  }
}

bool qtree_weight_supported(const int* Q, int D, int P, int T, int n_keys) {
  int off[QTREE_MAX_D + 2], boff[QTREE_MAX_D + 1];
  return qtree_layout(Q, D, off, boff) && P >= 0 && P <= QTREE_WEIGHT_MAX_TREES && T >= 0 && T <= 65535 &&
         n_keys >= 0 && n_keys <= QTREE_WEIGHT_MAX_KEYS;
}

int qtree_weight_segments(const int* row_ptr, int T, std::vector<int>& seg) {
  seg.clear();
  for (int t = 0; t < T; ++t) {
    const int n = row_ptr[t + 1] - row_ptr[t];
    for (int f = 0; f < n; f += QTREE_WEIGHT_SEG) { seg.push_back(t); seg.push_back(f); }
  }
  return (int)(seg.size() / 2);
}

int qtree_weight_plan(const int* trees, const double* coef, int P, int D, const int* off, std::vector<int>& meta,
                      std::vector<int>& ucols) {
  meta.clear(); ucols.clear();
  const int NN = off[D + 1];
  int Pa = 0;
  for (int p = 0; p < P; ++p) {
    int depth = -1;
    for (int l = 0; l <= D; ++l)
      for (int jn = off[l]; jn < off[l + 1]; ++jn)
        if (coef[(size_t)p * NN + jn] != 0.0) depth = l;
    if (depth < 0) continue;
    meta.push_back(p); meta.push_back(depth);
    for (int l = 1; l <= QTREE_MAX_D; ++l) {
      int slot = 0;
      if (l <= depth) {
        const int c = trees[(size_t)p * D + l - 1];
        for (slot = 0; slot < (int)ucols.size() && ucols[slot] != c; ++slot) {}
        if (slot == (int)ucols.size()) ucols.push_back(c);
      }
      meta.push_back(slot);
    }
    ++Pa;
  }
  return Pa;
}

size_t qtree_weight_lds_bytes(int tpp, int NN, int NB, int U) { return qw_carve(tpp, NN, NB, U).total; }

template <bool F32>
static void qw_launch_d(const QtreeWeightArgs& a, size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)a.nseg), block(QWNT);
  switch (a.D) {
    case 1: hipLaunchKernelGGL((k_qtree_weight<F32, 1>), grid, block, lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_qtree_weight<F32, 2>), grid, block, lds, st, a); break;
    case 3: hipLaunchKernelGGL((k_qtree_weight<F32, 3>), grid, block, lds, st, a); break;
    case 4: hipLaunchKernelGGL((k_qtree_weight<F32, 4>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((k_qtree_weight<F32, 5>), grid, block, lds, st, a); break;
  }
}

void launch_qtree_weight(const QtreeWeightArgs& a, hipStream_t st) {
  int off[QTREE_MAX_D + 2], boff[QTREE_MAX_D + 1];
  if (!qtree_weight_supported(a.Q, a.D, a.P, a.pv.T, a.U) || !qtree_layout(a.Q, a.D, off, boff) || a.Pa < 0 || a.Pa > a.P ||
      a.nseg < 0 || a.E < 0 || a.pv.F < 0 || a.tpp < 1 || a.tpp > QTREE_WEIGHT_MAX_TPP || (a.E > 0 && !a.extra) ||
      (a.Pa > 0 && a.nseg > 0 && (!a.seg || !a.meta || (a.U > 0 && !a.ucols) || !a.breaks || !a.count || !a.coef || !a.w_out)))
    dlap_throw_hip(hipErrorInvalidValue, "qtree_weight: unsupported arguments", __FILE__, __LINE__);
  if (a.nseg <= 0 || a.Pa <= 0) return;
  const size_t lds = qtree_weight_lds_bytes(a.tpp, off[a.D + 1], boff[a.D], a.U);
  if (lds > 64 * 1024) dlap_throw_hip(hipErrorInvalidValue, "qtree_weight: LDS image above 64 KiB", __FILE__, __LINE__);
  if (a.pv.fp32) qw_launch_d<true>(a, lds, st);
  else qw_launch_d<false>(a, lds, st);
  HIP_OK(hipGetLastError());
}
