// Characteristic knock-outs (k_knock.hip): the ensemble SDF of a split with a set of characteristic
// columns replaced by a base row, for many such scenarios from one read of the resident panel.
// Shared with the engine.
//
// Definition (analysis/knockout.py is the oracle). Scenario k is a set S_k of columns in [0, F)
// (a KP-bit mask, bit c of word c / 32) and a shared base row base[0..F-1]:
//   x^k[t,i,c] = base[c] for c in S_k, x[t,i,c] otherwise; the per-period columns are untouched.
// For member g of G in evaluation mode, per period t over its n_t valid rows:
//   w_g      raw tower output on x^k                                              (fp32)
//   c_g[t]   = fp32(S1_g[t] / max(n_t, 1)) if normalize_w else 0                  (fp64 quotient, rounded)
//   v_g      = w_g - c_g[t]                                                       (fp32)
//   SA_g[t]  = sum_i |v_g|     SR_g[t] = sum_i v_g R     S1_g[t] = sum_i w_g      (fp64)
//   s_g[t]   = fp32(1 / (G * max(fp32(SA_g[t]), 1e-8f)))                          (fp64 quotient, rounded)
//   e_i      = fma(v_G-1,i, s_G-1, ... fma(v_0,i, s_0, 0))                        (fp32, g ascending)
//   EA[t] = sum_i |e|    E2[t] = sum_i e^2    ER[t] = sum_i e R                   (fp64)
//   dense    = fp32(e / EA[t]) where EA[t] > 1e-8, else e                         (fp64 quotient, rounded)
//   n[t], sum_r[t] = sum_i R, sum_rr[t] = sum_i R^2                               (fp64, once per split)
#pragma once
#include "common.h"
#include "mlp.h"
#include "panel_view.h"

#define KNOCK_MAX_CHUNK 256          // scenarios per launch (their masks sit in LDS)
// Default bound of the raw-weight scratch wk [chunk][G][R] fp32 (Engine.knockout: max_scratch_bytes = 0)
#define KNOCK_DEFAULT_SCRATCH (256ull << 20)

struct KnockArgs {
  const uint32_t* masks;  // device [K][KP / 32]: the scenarios of this launch
  const float* base;      // device [KP]: the base row in panel columns, zero from F on
  int K, G, R, T;
  float* wk;              // [K][G][R] raw weights: written by k_knock_fwd, read by k_knock_reduce
};

struct KnockReduceArgs {
  PanelView pv;           // Rc, row_ptr, rowti, T, N are read
  const float* wk;        // [K][G][R]
  int K, G, R;
  int normalize_w;
  double* ens;            // [3][K][T]: EA, E2, ER
  double* mem;            // [3][K][G][T]: S1, SA, SR
  double* per;            // [3][T]: n, sum_r, sum_rr (written by the blocks of scenario 0), or null
  float* dense;           // [K][T][N] or null: written at the valid (t, i) only
};

// The fused layer-0 path (as sens_supported) whose LDS image -- the whole evaluation blob, aux, the
// T periods' inputs, the masks of a full chunk -- fits 160 KiB.
bool knock_supported(const MlpDims& D, int KS1, int T);
// jobs: the split's evaluation tower jobs of the G models (X, rowti, blob, aux, pp, R and T are
// read). Throws on an unsupported shape.
void launch_knock_fwd(const MlpJob* jobs, const KnockArgs& A, const MlpDims& D, int KS1, hipStream_t st);
void launch_knock_reduce(const KnockReduceArgs& A, hipStream_t st);
