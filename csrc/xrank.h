// Cross-sectional rank transform of a raw characteristic panel (k_xrank.hip): per (period,
// characteristic) the average-tie rank of the participating stocks, mapped into (-0.5, 0.5).
// data/transforms.py holds the definition (rank_characteristics_numpy, the oracle).
//
// Dense fp32 chunk x [T][N][F], rowok [T][N] (uint8). Element (t, i, f) participates iff rowok[t][i]
// and x > thr (a NaN compares false: missing; +inf participates). Over the participants A of (t, f),
// m = |A| -> cnt[t][f], and for i in A
//   lt = #{j in A : x_j < x_i},  eq = #{j in A : x_j == x_i}   (IEEE: -0 == +0; eq counts i)
//   out[t][i][f] = float(2 lt + eq - m) / float(2 m)            (one fp32 division, both operands exact)
// A missing element of a live row gets fill_missing, every element of a dead row fill_dead.
//
// Exactness. The kernel sorts the integer keys qkey_u32(x) of a column in LDS and reads lt and
// lt + eq off the sorted column by lower and upper bound, so every bit of out and cnt is a function
// of the column's data alone: not of the grid, the column blocking, T, or how a caller cuts the
// periods into chunks. No float atomics, no global atomics, no cross-workgroup wait, no scratch and
// no device memory besides the caller's buffers. out == x is legal: a workgroup owns its (period,
// column block) and every element is read and then written by one thread.
#pragma once
#include "common.h"

#define XRANK_MAX_N 32768           // one column's keys padded to a power of two, in LDS (128 KiB)

#ifndef XRANK_BLOCK_KEYS            // (-DXRANK_BLOCK_KEYS=n on k_xrank.hip: a side build for A/B runs) keys of a
#define XRANK_BLOCK_KEYS 8192       // workgroup while more than one column fits: a power of two (measured against
#endif                              // 4096 and 16384, profiles/rank_transform_timing.txt)
static_assert(XRANK_BLOCK_KEYS >= 8 && XRANK_BLOCK_KEYS <= XRANK_MAX_N && (XRANK_BLOCK_KEYS & (XRANK_BLOCK_KEYS - 1)) == 0,
              "XRANK_BLOCK_KEYS: a power of two in [8, XRANK_MAX_N]");

inline bool xrank_supported(int N) { return N >= 1 && N <= XRANK_MAX_N; }

// XRANK_BLOCK_KEYS as k_xrank.hip was compiled
int xrank_block_keys();

// Any F >= 1, any T >= 0 (more than 65535 periods go out in several launches), 1 <= N <= XRANK_MAX_N.
void launch_xrank(const float* x, const uint8_t* rowok, float* out, int* cnt, long long T, int N, int F,
                  float thr, float fill_missing, float fill_dead, hipStream_t st);
