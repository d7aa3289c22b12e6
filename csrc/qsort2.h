// Double-sorted portfolios on the resident panel (k_qsort2.hip): per period and pair of key
// columns (A, B), a Qa x Qb two-way quantile sort of the valid rows; per cell the row count and
// the fp64 sums of the value columns. Shared with the engine.
//
// Definition (analysis/sorted_portfolios.py, double_sort_numpy, is the oracle). The first key
// follows the single sort (qsort.h): s^A the n A-keys ascending (-0.0 == +0.0),
// bA_d = s^A[ceil(d n / Qa) - 1], d = 1..Qa-1, qa(i) = #{d : A_i > bA_d}. Independent mode: the
// same rule on B over all n rows with Qb. Conditional mode: for each first-key bucket a with
// n_a rows, s^{B|a} their B-keys ascending, bB_{a,d} = s^{B|a}[ceil(d n_a / Qb) - 1],
// qb(i) = #{d : B_i > bB_{qa(i),d}}; n_a = 0 leaves row a's cells empty and its breakpoints NaN.
// Tied keys share the lowest bucket any of them would get, in both dimensions.
#pragma once
#include "common.h"
#include "panel_view.h"

#define QSORT2_MAX_Q 16
#define QSORT2_MAX_CELLS 36     // Qa * Qb
#define QSORT2_MAX_VALUES 2     // caller-supplied value columns (value 0 is the split's return)

struct Qsort2Args {
  PanelView pv;           // the split's compacted panel (panel_view.h)
  // keys: index k < pv.F is panel column k, index pv.F + e the dense array e of extra
  int P;                  // pairs
  const int2* pairs;      // device [P] (A, B) key indices in [0, F + E)
  int Qa, Qb;             // 2 .. QSORT2_MAX_Q each, Qa * Qb <= QSORT2_MAX_CELLS
  int conditional;        // != 0: B's breakpoints within each A bucket; 0: over the whole period
  int E;
  const float* extra;     // device [E][T][N] fp32 (read at the valid rows only), or null when E == 0
  // values: Rc, then K dense arrays
  int K;                  // 0 .. QSORT2_MAX_VALUES
  const float* values;    // device [K][T][N] fp32, or null when K == 0
  // results, every element written by the launch
  int* count;             // [T][P][Qa][Qb]
  double* sum;            // [T][P][Qa][Qb][1+K]
  float* breaks_a;        // [T][P][Qa-1], NaN for an empty period
  float* breaks_b;        // [T][P][Qa][Qb-1], NaN where row a is empty (independent: Qa equal rows)
};

// One workgroup per (pair, period). Throws on Qa / Qb / K outside their ranges; T == 0 or P == 0
// launches nothing. The pair indices are the caller's to check (the engine does).
void launch_qsort2_port(const Qsort2Args& a, hipStream_t st);
