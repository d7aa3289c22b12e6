// Batched elastic-net coordinate descent along penalty paths (k_encd.hip): the pruning step of the
// asset-pricing trees. analysis/tree_prune.py holds the definition (en_paths_numpy, the oracle).
//
// A [NA][n][n] fp64, every matrix bitwise symmetric; per path p: the matrix a_of[p], b [P][n], the
// penalties l1s [P][n1] in the order they are run, l2 [P]. With M = A[a_of[p]], th = g = 0 at the
// start of the path and g carried along all of it, every point runs sweeps over j = 0 .. n-1 of
//   rho = b[j] - (g[j] - M[j][j] * th[j])
//   new = copysign(max(|rho| - l1, 0), rho) / (M[j][j] + l2)   (0 where M[j][j] + l2 <= 0)
//   d   = new - th[j];  if d != 0:  g[i] = g[i] + M[i][j] * d for all i,  th[j] = new
// until a sweep's largest |d| is <= 1e-10 max(1, max |th|) or max_sweeps sweeps are run. Every
// operation is one fp64 rounding (k_encd.hip is compiled with -ffp-contract=off), in this order.
//
// Exactness. A coordinate with d == 0 changes nothing, so the kernel evaluates d for all j >= j0 at
// once, takes the lowest j with d != 0, applies it and goes on from j + 1: the sequential loop's
// states in the sequential loop's order. theta, sweeps and nnz are a function of the path's inputs
// alone: not of the grid, of the other paths, of the workgroup size or of sweeps_per_launch.
// No atomics, no cross-workgroup wait, no scratch, no device memory besides the caller's buffers.
//
// Bounded launches. A launch runs at most sweeps_per_launch sweeps of a path, then leaves th, g,
// the point index, the sweep count and a done flag in the caller's state buffer; encd_run launches
// again until every path is done (one readback of 16 P bytes per launch).
#pragma once
#include <vector>
#include "common.h"

#define ENCD_MAX_N 4096             // th, g, b, diag(M) in LDS: 32 n bytes, + 4 n for the row hints

#ifndef ENCD_THREADS                // (-DENCD_THREADS=64 on k_encd.hip: a side build for A/B runs)
#define ENCD_THREADS 256            // measured against 64, profiles/tree_prune_timing.txt
#endif
#ifndef ENCD_PREFETCH               // (-DENCD_PREFETCH=0: every row is loaded when it is needed)
#define ENCD_PREFETCH 1
#endif
static_assert(ENCD_THREADS >= 64 && ENCD_THREADS <= 1024 && ENCD_THREADS % 64 == 0, "ENCD_THREADS: whole waves");

#define ENCD_DEFAULT_SWEEPS_PER_LAUNCH 256   // profiles/tree_prune_timing.txt

inline bool encd_supported(int n) { return n >= 1 && n <= ENCD_MAX_N; }

// state: [P][2][n] fp64 (th, g), then [P][4] int32 (point, sweeps of the point, done, updates so far)
inline size_t encd_state_bytes(long long P, int n) {
  return P < 0 || n < 0 ? 0 : (size_t)P * ((size_t)2 * n * sizeof(double) + 4 * sizeof(int));
}

int encd_threads();     // ENCD_THREADS / ENCD_PREFETCH as k_encd.hip was compiled
int encd_prefetch();

// theta [P][n1][n] fp64, sweeps and nnz [P][n1] int32 (points that are not computed stay 0), state
// encd_state_bytes(P, n); max_assets < 0: none. Zeroes state and outputs, launches until every path
// is done and returns the number of launches; ms (when given) gets the device time of each launch,
// updates the coordinate updates of each path (saturating at INT_MAX).
int encd_run(const double* A, const int* a_of, const double* b, const double* l1s, const double* l2, double* theta,
             int* sweeps, int* nnz, void* state, int NA, long long P, int n, int n1, int max_sweeps, int max_assets,
             int sweeps_per_launch, hipStream_t st, std::vector<float>* ms, std::vector<int>* updates);
