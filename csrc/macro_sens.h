// Macro importance through the LSTM (k_macro_sens.hip): the gradient of the scaled raw SDF weight
// with respect to the standardised macro series fed l periods before the row's period, reduced
// over the rows of a split. Shared with the engine.
#pragma once
#include "common.h"
#include "mlp.h"

struct PackLayer;

// One model of k_lstm_lagjac: the saved evaluation recurrence of the split.
struct LagJob {
  const float* params;    // flat fp32 parameter vector (W_hh of layer 0 is read from it)
  const float* sg;        // [T][4H] post-activation gates, PyTorch order i, f, g, o
  const float* sc;        // [T][H] cells
  const float* c0;        // [H] initial cell state of the split
};

struct MacroDims {
  int G, T, R;
  int L;                  // lags 0 .. L - 1 (L <= T); slot L of every period holds their sum
  int M, H;               // macro series, LSTM width (single layer)
  int w_ih, w_hh;         // flat offsets of W_ih [4H][M] and W_hh [4H][H]
};

// padded LSTM width of the kernels' layouts (4 or 8)
inline int macro_hm(int H) { return H <= 4 ? 4 : 8; }
// single-layer LSTM of H <= 8 units on the fused layer-0 path, where k_input_sens runs and the
// per-model state gradients of a round (G x 256 rows x HM floats) fit LDS beside its image
bool macro_sens_supported(const MlpDims& D, int KS1, int nrnn, int H, int G);
int macro_chunks(int R);                                   // a function of R only
size_t macro_c_floats(const MacroDims& A);                 // C [G][T][L + 1][HM][4][HM]
size_t macro_part_floats(const MacroDims& A);              // chunk partials
size_t macro_out_doubles(const MacroDims& A);              // [G L + L + 1][M]

// C[g][t][l][k][q][j] = d h_t[k] / d pre_{t-l}[gate q, unit j] (zero where t - l < 0, and in the
// padding k, j >= H); slot l = L: the sum over the lags present. C must be zero-filled.
void launch_lstm_lagjac(const LagJob* jobs, const MacroDims& A, float* C, hipStream_t st);

// jobs / sj as for launch_input_sens. out (fp64): rows g L + l = sum_rows |prod_g,l| [M], rows
// G L + l (l <= L) = sum_rows |sum_g prod_g,l| (l = L: the lag-summed response).
void launch_macro_sens(const MlpJob* jobs, const SensJob* sj, const MacroDims& A, const MlpDims& D, int KS1,
                       const PackLayer& L0, const float* C, float* part, double* out, hipStream_t st);
