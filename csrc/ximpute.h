// Cross-sectional factor imputation of missing characteristics (k_ximpute.hip): the masked second
// moments of a ranked chunk and the per-row ridge fit that fills its holes.
// data/transforms.py holds the definitions (characteristic_moments_numpy, xs_loadings,
// xs_fill_numpy: the oracles).
//
// Dense fp32 chunk y [T][N][F], rowok [T][N] (uint8). Element (t, i, f) is observed, o = 1, iff
// rowok[t][i] and y == y (a NaN marks a hole); z = y where observed, else 0. Dead rows and holes may
// hold anything: they are selected to 0, never multiplied.
//
//   k_ximp_gram   S[t][a][b] = sum_i z_ia z_ib (fp64), C[t][a][b] = sum_i o_ia o_ib (int32).
//   k_ximp_fill   per live row, with the period's loadings lam [F][K] (fp32, K <= XIMP_MAX_K):
//                   A = gamma I + sum_{f observed} lam_f lam_f',  b = sum_{f observed} lam_f y_f,  g = A^-1 b,
//                   out[t][i][f] = clip(lam_f . g, -0.5, 0.5) for every f not observed;
//                 observed entries and dead rows keep their bits.
//
// Determinism. A period's stocks are cut into runs of XIMP_RUN consecutive stock indices counted from
// stock 0. S[t] is the sum, in run order, of the fp32 moments of each run: inside a run the stocks
// are the MFMA k axis, walked 32 at a time in a fixed order with fp32 accumulation of exact
// fp32 x fp32 products; each run's fp32 tile is converted to fp64 and added to fp64 accumulators
// in registers. The indicator products run on the bf16 MFMA and are exact (a run's counts stay below
// 2^24); each run's counts are folded into int32. The bits of S and C depend on the period's data
// only: not on the grid, on T, or on how a caller chunks the periods. The lower triangles are bitwise
// mirrors (only tile pairs a <= b are computed). A filled row depends on that row and lam[t] only.
// No atomics, no scratch, no cross-workgroup wait and no device memory besides the caller's
// buffers. out == y is legal for the fill: a wave owns its rows and reads a row before it writes it.
#pragma once
#include "common.h"

#ifndef XIMP_RUN                // (-DXIMP_RUN=n on k_ximpute.hip: a side build for A/B runs) stocks per fp32
#define XIMP_RUN 128            // run: a multiple of 64, <= 512 (k_xgram's measured choice)
#endif
static_assert(XIMP_RUN >= 64 && XIMP_RUN <= 512 && XIMP_RUN % 64 == 0, "XIMP_RUN: a multiple of 64 in [64, 512]");

#define XIMP_MAX_K 8            // loadings per characteristic the fill kernel is instantiated for
#define XIMP_LDS_MAX (160 * 1024)

// LDS image of k_ximp_fill: the period's table [F rounded up to 32][lam | vech(lam lam') | pad] and
// a transposition buffer of 64 rows per wave.
inline int ximp_table_cols(int K) { return ((K + K * (K + 1) / 2 + 15) / 16) * 16; }
inline size_t ximp_fill_lds(int F, int K) {
  const int nc = ximp_table_cols(K);
  return ((size_t)((F + 31) / 32 * 32) * (nc + 2) + (size_t)4 * 64 * (nc + 1)) * sizeof(float);
}
// F characteristics with K loadings each (K the number of columns of lam, min(K, F) of the caller's
// request): 1 <= F <= 512 with 1 <= K <= 8 always fit.
inline bool ximp_supported(int F, int K) {
  return F >= 1 && K >= 1 && K <= XIMP_MAX_K && ximp_fill_lds(F, K) <= XIMP_LDS_MAX;
}

// XIMP_RUN as k_ximpute.hip was compiled
int ximp_run();

// Any N >= 1, any T >= 0 (more than 65535 periods go out in several launches), ximp_supported(F, 1).
// S [T][F][F] double, C [T][F][F] int32; every element is written.
void launch_ximp_gram(const float* y, const uint8_t* rowok, double* S, int* C, long long T, int N, int F,
                      hipStream_t st);

// lam [T][F][K] fp32, ximp_supported(F, K), gamma > 0. out may be y.
void launch_ximp_fill(const float* y, const uint8_t* rowok, const float* lam, float* out, long long T, int N,
                      int F, int K, float gamma, hipStream_t st);
