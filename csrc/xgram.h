// Per-period characteristic Gram on the resident panel (k_xgram.hip): the second-order statistic
// behind the factor benchmarks (IPCA, Fama-MacBeth). Shared with the engine.
// analysis/ipca.py holds the definitions (numpy, the oracle).
//
// Per period t of a split, over its valid rows, with x as the engine stores it:
//   gram[t][a][b] = sum_i x[i][a] x[i][b]  (a, b < F),  sum_r[t] = sum R,  sum_rr[t] = sum R^2,
//   n[t] from row_ptr.
// The kernel reads the resident panel only (panel_view.h: X, Rc and row_ptr), so it runs for every
// engine shape (fused and wide layer-0 path, bf16 and fp32 panel) and needs no model.
//
// Determinism. A period is cut into runs of XGRAM_RUN consecutive rows counted from its first row
// (the partition depends on row_ptr alone). gram[t] is the sum, in run order, of the fp32 Gram of
// each run: inside a run the rows are the MFMA k axis, walked 32 at a time in a fixed order with
// fp32 accumulation of exact products (bf16 x bf16 and fp32 x fp32 operands of the fp32-result
// MFMAs); each run's fp32 tile is converted to fp64 and added to fp64 accumulators that stay in
// registers while a workgroup walks its period. No float atomics and no scratch: the bits depend
// on row_ptr and the data only, not on the grid or on how tiles are spread over waves.
// The lower triangle is a bitwise mirror of the upper one (only tile pairs a <= b are computed).
#pragma once
#include <vector>
#include "common.h"
#include "panel_view.h"

#ifndef XGRAM_RUN               // (-DXGRAM_RUN=n on k_xgram.hip: a side build for A/B runs; the engine
#define XGRAM_RUN 128           // asks xgram_run()) rows per fp32 run: a multiple of 32, <= 512 (measured
#endif                          // against 32 and 512, profiles/ipca_timing.txt)
static_assert(XGRAM_RUN >= 32 && XGRAM_RUN <= 512 && XGRAM_RUN % 32 == 0, "XGRAM_RUN: a multiple of 32 in [32, 512]");

struct XgramArgs {
  PanelView pv;           // the split's compacted panel (panel_view.h; rowti and N are not read)
  // super-tiles (xgram_tiles): (ia, ib) = feature blocks 2 ia, 2 ia + 1 against 4 ib .. 4 ib + 3
  const int2* tiles;
  int ntiles;
  // results
  double* gram;           // [T][F][F]
  double* sum_r;          // [2][T] (sum_r, sum_rr)
  int* n;                 // [T]
};

// The super-tiles that meet the upper triangle of the ceil(F / 16)^2 tile grid, as (ia, ib) pairs
// ordered by ib then ia, so the four waves of a workgroup share their column blocks.
void xgram_tiles(int F, std::vector<int>& tiles);

// XGRAM_RUN as k_xgram.hip was compiled
int xgram_run();

// T == 0 launches nothing (the caller's zero-filled results stand).
void launch_xgram(const XgramArgs& a, hipStream_t st);
