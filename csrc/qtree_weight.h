// Stock-level weights of a combination of tree nodes on the resident panel (k_qtree_weight.hip): a
// node of a tree sort (qtree.h) is an equally weighted basket, so a coefficient table over the nodes
// of P trees is a weight per stock-month. Every valid row is walked down every tree that carries a
// non-zero coefficient and collects coef / node size at each node of its path. Shared with the engine.
//
// Definition (analysis/tree_sorts.py, tree_weights_numpy, is the oracle). With the layout of qtree.h,
// breaks [T][P][NB] and count [T][P][NN] of a tree sort of the same keys and coef fp64 [P][NN]
// (finite; -0.0 is read as 0), a valid row (t, i) has, per tree p, node_0 = 0 and
//   node_l = node_{l-1} Q_l + #{d : key_{c_l} + 0 > b_{node_{l-1}, d}},  l = 1..D
// (keys and breakpoints compared as floats, -0.0 == +0.0, nothing is above a NaN breakpoint), and
//   acc = +0.0;  for p ascending, l = 0..D ascending, j = off[l] + node_l:
//     if coef[p][j] != 0:  acc = acc + coef[p][j] / count[t][p][j]        (fp64, each rounded once)
//   w[t][i] = float(acc)
// acc is never -0.0, so adding the +0.0 of a zero coefficient changes no bit: the kernel drops the
// trees whose coefficient row is zero, stops a tree at its deepest non-zero level and adds the
// table entry coef / count (0.0 where coef == 0) of every node it does visit.
//
// Limits (qtree_weight_supported): those of k_qtree_port (D <= 5, at most 36 leaves, T <= 65535, at
// most 4096 trees per call) and at most QTREE_WEIGHT_MAX_KEYS distinct key columns among the
// active levels of a call: the keys of a segment are staged once in LDS, 1 KiB per key.
#pragma once
#include <vector>
#include "common.h"
#include "panel_view.h"
#include "qtree.h"

// Rows per segment = threads per workgroup: one lane per row.
#ifndef QTREE_WEIGHT_SEG
#define QTREE_WEIGHT_SEG 256
#endif
#define QTREE_WEIGHT_MAX_KEYS 32        // distinct key columns of a call (32 KiB of LDS)
#define QTREE_WEIGHT_MAX_TREES 4096
#define QTREE_WEIGHT_DEFAULT_TPP 16     // trees per pass (measured: profiles/tree_weights_timing.txt)
#define QTREE_WEIGHT_MAX_TPP 32         // 32 x (72 x 8 + 36 x 4) B of tables + the keys stay under 64 KiB
#define QTREE_WEIGHT_META (2 + QTREE_MAX_D)   // ints per active tree: tree, depth, key slot of every level

struct QtreeWeightArgs {
  PanelView pv;           // the split's compacted panel (panel_view.h)
  const int2* seg;        // [nseg] (period, first row of the segment within it), qtree_weight_segments
  int nseg;
  // the call compacted by the host (qtree_weight_plan)
  int Pa;                 // active trees, in the caller's order
  const int* meta;        // device [Pa][QTREE_WEIGHT_META]: the tree's index in [0, P), its deepest active
                          // level in [0, D], the LDS slot in [0, U) of its level-l key (0 beyond the depth)
  int U;                  // distinct key columns, <= QTREE_WEIGHT_MAX_KEYS
  const int* ucols;       // device [U] key indices in [0, F + E): k < pv.F panel column k, else extra k - F
  int P, D;               // trees of the tables; levels
  int Q[QTREE_MAX_D];
  int E;
  const float* extra;     // device [E][T][N] fp32 (read at the valid rows only), or null when E == 0
  const float* breaks;    // device [T][P][NB]
  const int* count;       // device [T][P][NN]
  const double* coef;     // device [P][NN]
  int tpp;                // trees per pass, 1 .. QTREE_WEIGHT_MAX_TPP
  // results, written at the valid (t, i) only
  float* w_out;           // dense [T][N]
  double* acc_out;        // dense [T][N] or null
};

// D, Q within the tree sort's ranges, P trees, T periods and n_keys distinct key columns
bool qtree_weight_supported(const int* Q, int D, int P, int T, int n_keys);

// The segment table of a split from the host copy of row_ptr [T+1]: (period, first row within it)
// pairs, QTREE_WEIGHT_SEG rows each (the last of a period shorter). Returns the number of segments.
int qtree_weight_segments(const int* row_ptr, int T, std::vector<int>& seg);

// Compacts a call: trees [P][D] key indices, coef [P][NN] -> meta [Pa][QTREE_WEIGHT_META] and the
// distinct key columns ucols of the active levels, in the order of first use. Returns Pa.
int qtree_weight_plan(const int* trees, const double* coef, int P, int D, const int* off, std::vector<int>& meta,
                      std::vector<int>& ucols);

// Dynamic LDS of a launch
size_t qtree_weight_lds_bytes(int tpp, int NN, int NB, int U);

// One workgroup per segment. Throws on arguments outside qtree_weight_supported; nseg == 0 or
// Pa == 0 launches nothing.
void launch_qtree_weight(const QtreeWeightArgs& a, hipStream_t st);
