// Linear benchmark SDFs on the resident panel (k_linport.hip): the characteristic-managed sums
// of a split and the per-period sums of up to LINPORT_MAX_K linear portfolios w = x . theta_k.
// Shared with the engine. analysis/benchmarks.py holds the definitions (numpy, the oracle).
//
// Both kernels read the resident panel only (panel_view.h: X, Rc and row_ptr; k_linport also rowti
// when it writes the dense weights), so they run for every engine shape. A period is cut into
// segments of LINPORT_SEG rows (a constant: the partition depends on row_ptr alone); a workgroup
// owns one segment, and the segments of a period are added in index order by a second small
// launch. fp64 sums, no float atomics: repeated calls are bitwise identical.
//
//   k_managed   sum_x[t][f] = sum_i x, sum_xr[t][f] = sum_i x R over the valid rows of period t.
//   k_linport   per (t, k), with w = x . theta_k on v_mfma_f32_16x16x4_f32 (bf16 panel values
//               convert to fp32 exactly; fp32 products and accumulation), c = center[t][k] (0
//               when absent) and v = fp32(w - c):
//                 S1 = sum (v + c), SA = sum |v|, S2 = sum v^2, SR = sum v R    (fp64)
//               and per t: sum_r = sum R, sum_rr = sum R^2. S1 is formed from v so that all four
//               sums describe exactly the fp32 values written to w_out (S1 - n c = sum v); with
//               c = 0 it is sum w.
#pragma once
#include <vector>
#include "common.h"
#include "panel_view.h"

#define LINPORT_MAX_K 64
// Rows per segment (32 MFMA row tiles; measured against 256 and 1024,
// profiles/linear_benchmarks_timing.txt). A side build for A/B runs sets -DLINPORT_SEG=n on
// k_linport.hip and k_pred.hip, the two files that compile it in; the engine asks linport_segments.
#ifndef LINPORT_SEG
#define LINPORT_SEG 512
#endif

struct LinportArgs {
  PanelView pv;           // the split's compacted panel (panel_view.h)
  // segments (linport_segments): seg[j] = (period, first row of the segment within it),
  // seg_ptr[t] .. seg_ptr[t+1] the segments of period t
  const int2* seg;
  const int* seg_ptr;
  int nseg;
  // k_linport
  int K;                  // candidates, 1 .. LINPORT_MAX_K
  const float* theta;     // packed operand fragments, linport_theta_floats(F, K) floats (linport_pack_theta)
  const float* center;    // [T][K] fp32 or null
  float* w_out;           // dense [K][T][N] fp32 or null: v is written at the valid (t, i) only
  double* part;           // [nseg][4][16 NV] (k_linport) or [nseg][2][F] (k_managed) segment partials
  double* part_r;         // [nseg][2] (k_linport)
  // results
  double* out;            // k_linport: [4][T][K] (S1, SA, S2, SR); k_managed: [2][T][F] (sum_x, sum_xr)
  double* out_r;          // k_linport: [2][T] (sum_r, sum_rr)
  int* n;                 // [T]
};

// 16-candidate blocks of a launch (1, 2 or 4) and the packed size of theta
int linport_nv(int K);
size_t linport_theta_floats(int F, int K);
// theta [K][F] -> the B-operand fragments the kernel stages in LDS: element
// ((s * 64 + lane) * NV + v) = theta[16 v + (lane & 15)][16 (s / 4) + 4 (lane / 16) + s % 4], 0 beyond K / F
void linport_pack_theta(const float* theta, int K, int F, float* packed);
// true when the fragments of an F-column theta fit the LDS of a workgroup
bool linport_supported(int F);
size_t linport_part_doubles(int nseg, int K);
// The segment table of a split from the host copy of row_ptr [T+1], cut as k_linport.hip was
// compiled: seg = (period, first row within it) pairs, seg_ptr [T+1]. Returns the number of segments.
int linport_segments(const int* row_ptr, int T, std::vector<int>& seg, std::vector<int>& seg_ptr);

// T == 0 or nseg == 0 launches nothing (the caller's zero-filled results stand).
void launch_managed(const LinportArgs& a, hipStream_t st);
void launch_linport(const LinportArgs& a, hipStream_t st);
