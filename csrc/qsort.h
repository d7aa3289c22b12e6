// Characteristic-sorted portfolios on the resident panel (k_qsort.hip): per period and key column,
// the Q - 1 quantile breakpoints of the valid rows' keys (exact order statistics), every row's
// bucket, and per bucket the row count and the fp64 sums of the value columns. Shared with the
// engine.
//
// Definition (analysis/sorted_portfolios.py is the oracle): the period's n keys sorted ascending
// are s[0..n-1] (-0.0 == +0.0); b_d = s[ceil(d n / Q) - 1], d = 1..Q-1; bucket(i) = #{d : key_i > b_d}.
// Tied keys share the lowest bucket any of them would get.
#pragma once
#include "common.h"
#include "panel_view.h"

#define QSORT_MAX_Q 16
#define QSORT_MAX_VALUES 4      // caller-supplied value columns (value 0 is the split's return)

struct QsortArgs {
  PanelView pv;           // the split's compacted panel (panel_view.h)
  // keys: C characteristic columns (cols[k], or k when cols is null), then E dense arrays
  int Q;                  // buckets, 2 .. QSORT_MAX_Q
  int C;
  const int* cols;        // device [C] or null
  int E;
  const float* extra;     // device [E][T][N] fp32 (read at the valid rows only), or null when E == 0
  // values: Rc, then K dense arrays
  int K;                  // 0 .. QSORT_MAX_VALUES
  const float* values;    // device [K][T][N] fp32, or null when K == 0
  // results, every element written by the launch
  int* count;             // [T][C+E][Q]
  double* sum;            // [T][C+E][Q][1+K]
  float* breaks;          // [T][C+E][Q-1], NaN for an empty period
};

// One workgroup per (key, period). Throws on Q / K outside their ranges; T == 0 or C + E == 0
// launches nothing.
void launch_qsort_port(const QsortArgs& a, hipStream_t st);
