// Job record of the moment network's macro LSTM (k_mlstm.hip; config key `moment_lstm`).
//
// The moment towers see the macro series only through the per-period layer-0 bias table
// abias[T][64]. With the moment LSTM on, the table is W_m0[:, :Hm] . hm_t + b_m0 with
// hm = LSTM(macro) (one layer, width Hm <= 32, zero initial state), and phase 2's gradient of
// the table, dab[T][64], is carried back through the recurrence to the LSTM tensors at the
// head of the flat vector's moment segment.
#pragma once
#include "common.h"

struct ModelDesc;

#define DLAP_MAX_MH 32       // max moment-LSTM width on the GPU

struct MlstmJob {
  const float* params;   // flat parameters of this job's model
  float* grads;          // flat gradients (backward)
  const float* macro;    // [T][M] standardised macro series of the split
  int T;
  float* xg;             // [T][4Hm] input projections (W_ih m_t + b_ih + b_hh)
  float* hm;             // [T][Hm] LSTM outputs (always written: the table's operand)
  float* sg;             // train: saved post-activation gates [T][4Hm] (nullptr: not saved)
  float* sc;             // train: saved cells [T][Hm]
  float* abias;          // [T][64] moment layer-0 per-period bias
  const float* dab;      // backward: [T][64] gradient of abias (live columns c < cm1)
  float* dg;             // backward: [T][4Hm] gate pre-activation gradients
  float* dhm;            // backward: [T][Hm] gradient of hm from the table
};

// xg, the recurrence and the table abias of every job. train: save gates / cells for the backward.
void launch_mlstm_fwd(const MlstmJob* jobs, int njobs, int tmax, const ModelDesc* md, const ModelDesc& mh,
                      hipStream_t st, bool train);

// Phase 2, after k_finalize has written dab: db_m0, dW_m0[:, :Hm], BPTT, and the LSTM tensors'
// gradients into the flat gradient vector (two launches, stream ordered).
void launch_mlstm_bwd(const MlstmJob* jobs, int njobs, int tmax, const ModelDesc* md, const ModelDesc& mh,
                      hipStream_t st);
