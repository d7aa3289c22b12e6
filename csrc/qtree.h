// Tree-sorted portfolios on the resident panel (k_qtree.hip): per period and tree (c_1, .., c_D)
// of key indices, D nested conditional quantile splits Q_1, .., Q_D of the valid rows; per node of
// every level the row count and the fp64 sums of the value columns. Shared with the engine.
//
// Definition (analysis/tree_sorts.py, tree_sort_numpy, is the oracle). Level 0 is the root with
// all n rows; level l >= 1 has n_l = Q_1 .. Q_l nodes. For a node a of level l - 1 with m_a rows,
// s their c_l keys ascending (-0.0 == +0.0): b_{a,d} = s[ceil(d m_a / Q_l) - 1], d = 1..Q_l-1, and
// a row of the node goes to child a Q_l + #{d : key > b_{a,d}}. Tied keys share the lowest child
// any of them would get. m_a = 0 leaves the node's breakpoints NaN and its subtree empty. D = 1 is
// the single sort (qsort.h), D = 2 the conditional double sort (qsort2.h).
//
// Layout (level order): off[l] = n_0 + .. + n_{l-1}, node (l, j) at off[l] + j, NN = off[D+1];
// boff[l] = sum_{k<l} n_k (Q_{k+1} - 1), breakpoint (l, a, d), l = 1..D, at
// boff[l-1] + a (Q_l - 1) + (d - 1), NB = boff[D] = L - 1 with L = n_D the number of leaves.
#pragma once
#include "common.h"
#include "panel_view.h"

#define QTREE_MAX_Q 16
#define QTREE_MAX_LEAVES 36     // Q_1 .. Q_D
#define QTREE_MAX_D 5           // (2^5 = 32 <= 36 < 2^6)
#define QTREE_MAX_VALUES 2      // caller-supplied value columns (value 0 is the split's return)
#define QTREE_MAX_NODES 72      // NN <= 2 L - 1 (every level at most half the next)

struct QtreeArgs {
  PanelView pv;           // the split's compacted panel (panel_view.h)
  // keys: index k < pv.F is panel column k, index pv.F + e the dense array e of extra
  int P;                  // trees
  const int* trees;       // device [P][D] key indices in [0, F + E)
  int D;                  // 1 .. QTREE_MAX_D
  int Q[QTREE_MAX_D];     // 2 .. QTREE_MAX_Q each, product <= QTREE_MAX_LEAVES
  int E;
  const float* extra;     // device [E][T][N] fp32 (read at the valid rows only), or null when E == 0
  // values: Rc, then K dense arrays
  int K;                  // 0 .. QTREE_MAX_VALUES
  const float* values;    // device [K][T][N] fp32, or null when K == 0
  // results, every element written by the launch
  int* count;             // [T][P][NN]
  double* sum;            // [T][P][NN][1+K]
  float* breaks;          // [T][P][NB], NaN where the period or the node is empty
};

// off [D+2] and boff [D+1] of the layout above; returns false for splits outside the ranges
inline bool qtree_layout(const int* Q, int D, int* off, int* boff) {
  if (D < 1 || D > QTREE_MAX_D) return false;
  int n = 1;
  off[0] = 0; off[1] = 1; boff[0] = 0;
  for (int l = 1; l <= D; ++l) {
    if (Q[l - 1] < 2 || Q[l - 1] > QTREE_MAX_Q) return false;
    boff[l] = boff[l - 1] + n * (Q[l - 1] - 1);
    n *= Q[l - 1];
    if (n > QTREE_MAX_LEAVES) return false;
    off[l + 1] = off[l] + n;
  }
  return true;
}

// One workgroup per (tree, period). Throws on D / Q / K outside their ranges; T == 0 or P == 0
// launches nothing. The key indices are the caller's to check (the engine does).
void launch_qtree_port(const QtreeArgs& a, hipStream_t st);
