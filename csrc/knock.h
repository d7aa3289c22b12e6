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
//
// Macro knock-outs (Engine.knockout_macro). A scenario also holds a set Q_k of macro series in
// [0, M) (an M-bit mask) and the shared base row macro_base[0..M-1] (the standardised series the
// model is fed; zero is the training mean):
//   m^k[t][j] = macro_base[j] for j in Q_k and every period t of the split, m[t][j] otherwise;
//   pp_g^k    = member g's evaluation LSTM run over m^k[0..T-1] from the state the split's
//               evaluation starts from (every layer, evaluation mode); without an LSTM pp_g^k = m^k;
//   w_g       = raw tower output on (x^k, pp_g^k); everything after it is the definition above.
// A series is held constant over the whole split: no windows, no lags. The moment network, the
// train statistics and the split's length are untouched. Per chunk of scenarios:
// k_knock_macro_fill writes the altered series of the scenarios with a non-empty Q_k, the
// forward's own k_proj / recurrence kernels (launch_prologue) turn them into one [T][Dm] table
// per (scenario, member), and k_knock_fwd_pp evaluates the towers with the scenario's table
// inserted into tiles it loaded once. A scenario with an empty Q_k reads the split's own table.
// Out of scope: windows or lags, the state columns of an LSTM model, sharing a recurrence between
// scenarios, the moment network's LSTM, retraining, the wide layer-0 path, multi-rank runs.
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

// k_knock_fwd_pp: the tower pass with one per-period table per (scenario, member)
struct KnockPpArgs {
  KnockArgs a;
  const float* const* tabs;  // device [K][G]: fp32 [T][Dm] per-period inputs of (scenario, member)
};

// k_knock_macro_fill: the macro series of U scenarios with their Q_k replaced by the base row
struct KnockFillArgs {
  const float* macro;     // [T][M] the split's standardised series
  const uint32_t* masks;  // device [U][(M + 31) / 32]
  const float* base;      // device [M]
  float* out;             // [U][stride] floats: copy u is [T][M] at out + u * stride
  size_t stride;          // floats between copies: a multiple of 4 (16-byte aligned copies)
  int U, T, M;
};
// floats between the copies of k_knock_macro_fill
inline size_t knock_fill_stride(int T, int M) { return ((size_t)T * M + 3) & ~(size_t)3; }

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
// knock_supported, and the LDS image of k_knock_fwd_pp (blob, aux, masks, table pointers) fits too
bool knock_pp_supported(const MlpDims& D, int KS1, int T);
// the same tower pass with the [ppc, ppc + Dm) columns of every scenario taken from its table
// (A.tabs); shapes as launch_knock_fwd. With Dm = 0 the tables are not read.
void launch_knock_fwd_pp(const MlpJob* jobs, const KnockPpArgs& A, const MlpDims& D, int KS1, hipStream_t st);
void launch_knock_macro_fill(const KnockFillArgs& A, hipStream_t st);
