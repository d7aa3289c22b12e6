// SDF weight structure (k_wsurf.hip): the raw SDF weight of hypothetical stocks whose feature row
// is a base row with one or two characteristics moved over a grid, summed over the periods of a
// split and the models of an ensemble. Shared with the engine.
//
// Definition (analysis/weight_structure.py is the oracle): items (a, b), curves (b = -1) first,
// then surfaces; grid u[0..P-1]; base row x0[0..F-1]; scale table s[g][t]:
//   curve  (a)    [p]    = sum_g sum_t s[g][t] * w_g(x0 with x[a] = u[p]             , pp_g[t])
//   surface(a, b) [p][q] = sum_g sum_t s[g][t] * w_g(x0 with x[a] = u[p], x[b] = u[q], pp_g[t])
// w_g the evaluation-mode raw tower output, pp_g[t] the per-period inputs of model g. The rows
// are the concatenated points of the items: P per curve, P * P per surface with q fastest.
#pragma once
#include "common.h"
#include "mlp.h"

#define WSURF_MAX_P 64

struct WsurfArgs {
  const float* scale;     // device [G][T]
  const float* grid;      // device [P]
  const float* base;      // device [KP]: the base row in panel columns, zero from F on
  const int2* items;      // device [n1 + n2] (a, b): n1 curves (b = -1), then n2 surfaces
  int n1, n2, P;
  int rows;               // n1 P + n2 P P
  int G, T;
  float* out;             // [rows], every element written by the launch
};

// The launch's chunking (chosen from the number of 32-row tiles and the device's SIMDs; the values
// do not depend on it): period_split waves share a tile's periods (1, 2, 4 or 8), or a wave owns
// tiles_per_wave tiles (1 or 2).
struct WsurfPlan {
  int period_split, tiles_per_wave;
};

// The fused layer-0 path (as sens_supported) whose LDS image -- the whole evaluation blob, aux,
// the T periods' inputs, one model's T scales and period list, 2 KiB of exchange buffer -- fits
// 160 KiB.
bool wsurf_supported(const MlpDims& D, int KS1, int T);
// jobs: the split's evaluation tower jobs of the G models (blob, aux, pp and T are read; the panel
// is not). Throws on an unsupported shape.
WsurfPlan launch_weight_surface(const MlpJob* jobs, const WsurfArgs& A, const MlpDims& D, int KS1, hipStream_t st);
