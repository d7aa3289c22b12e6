// Prediction towers on the resident panel (k_pred.hip): the squared-error loss of the raw tower
// output against a per-row target, and the device-side bookkeeping of a fit epoch. Shared with
// the engine. analysis/prediction.py holds the definition (numpy, the oracle).
//
// For the compact rows r = (t, i) of a split, raw tower output p[r], returns R[r] and an optional
// per-period factor f[t] (absent: 1):
//   y = fp32(R * f[t]),  e = fp32(p - y),  dw[r] = 2.f * c[t] * e   (fp32, one rounding)
//   per period (fp64): SE = sum e^2, SY = sum y^2, S1 = sum p, SA = sum |p|, S2 = sum p^2, SR = sum p R
//   loss = sum_t (double)c[t] * SE[t]
// c[t] is the host-built weight of a row of period t (it depends on row_ptr only): "period"
// weighting fp32(1 / (T' n_t)) with T' the non-empty periods, "pooled" fp32(1 / R).
//
// A period is cut into segments of LINPORT_SEG rows (the segment table of the linear benchmarks:
// the partition depends on row_ptr alone); a workgroup of k_pred_loss owns one segment of one
// model, k_pred_end adds the segments of a period in index order. fp64 sums in a fixed order, no
// float atomics: repeated calls are bitwise identical, and a model's results do not depend on
// the models batched beside it. Neither kernel waits on anything: every hand-off is stream order.
#pragma once
#include "common.h"
#include "linport.h"

enum { PRED_SE = 0, PRED_SY, PRED_S1, PRED_SA, PRED_S2, PRED_SR, PRED_NSUM = 6 };
// History row written per fit epoch by k_pred_end (PRED_HIST_W floats)
enum { PH_TRAIN_LOSS = 0, PH_VALID_LOSS, PH_TEST_LOSS, PH_GNORM, PH_BEST, PRED_HIST_W = 5 };

struct PredJob {           // one model, one split
  const float* w;          // [R] raw tower output
  float* dw;               // [R] dL/dw (written when PredArgs::write_dw)
  double* part;            // [nseg][PRED_NSUM] segment partials
};

struct PredArgs {          // one split
  const PredJob* jobs;     // [models]
  const float* Rc;         // [R]
  const float* f;          // [T] or null (ones)
  const float* c;          // [T] row weights
  const int* row_ptr;      // [T+1]
  const int2* seg;         // [nseg] (period, first row of the segment within it)
  int nseg;
  int write_dw;
};

struct PredSplit {         // one (model, split) of the bookkeeping
  const double* part;      // [nseg][PRED_NSUM] (PredJob::part)
  double* sums;            // [PRED_NSUM][T] per-period sums of the last pass
  const float* c;          // [T]
  const int* seg_ptr;      // [T+1] segments of period t
  int T;
};

struct PredEndJob {        // one model
  PredSplit sp[3];
  double* loss;            // [3] loss of the last pass of each split
  float* hist;             // [max_ep][PRED_HIST_W]
  int* ep;                 // [2] fit epoch counter, best epoch (-1: none)
  float* best;             // [1] best validation loss
  const float* gnorm;      // pre-clip gradient norm of the epoch's update
  const float* params;
  float* snap;             // [P] parameters at the best validation loss
  const int* prog;         // as UpdJob::prog: a poisoned model records NaN, takes no snapshot
  int max_ep;              // rows of hist: epochs past the capacity are not recorded
};

// nseg == 0 launches nothing.
void launch_pred_loss(const PredArgs& a, int njobs, hipStream_t st);
// smask: the splits (bit s) whose partials this launch reduces into sums / loss. book: also the
// epoch's history row, best tracker and snapshot (valid split: bit 1 of smask), and the counter.
void launch_pred_end(const PredEndJob* jobs, int njobs, int smask, int book, int P, hipStream_t st);
// best = +inf, best epoch = -1, epoch counter = 0 (stream-ordered)
void launch_pred_begin(const PredEndJob* jobs, int njobs, hipStream_t st);
