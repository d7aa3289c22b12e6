// Prediction towers on the resident panel (pred.h): the squared-error loss of the raw tower
// output and the bookkeeping of a fit epoch.
//
//   k_pred_loss      grid (segments, models), 256 threads. A thread takes rows tid, tid + 256, .. of
//                    its segment (adjacent lanes adjacent rows: coalesced loads of w and Rc, coalesced
//                    stores of dw), forms y, e and dw in fp32 with single roundings and adds the
//                    six sums in fp64. Lanes by a fixed xor tree (32 .. 1), the four waves in order
//                    through LDS, one partial per (model, segment). It reads no feature rows: the
//                    same kernel serves bf16 / fp32 panels and the fused / wide layer-0 paths.
//   k_pred_end       grid (models), 1024 threads. Per split of the launch's mask: thread t adds the
//                    segment partials of period t in segment order and writes the per-period sums;
//                    loss = sum_t (double)c[t] SE[t] (periods t, t + 1024, .. within a thread, then the
//                    xor tree and the waves in order). With `book`, thread 0 then writes the epoch's
//                    history row and moves the best tracker (strictly lower validation loss; NaN
//                    never wins; a poisoned model records NaN), and the block copies the parameters
//                    into the snapshot when the epoch is the best so far.
// These launches move a few MB and are latency-bound; neither spins or waits on another launch.
#include <cmath>
#include "common.h"
#include "pack_dev.h"
#include "pred.h"

namespace {

constexpr int kNT = 256;
constexpr int kWaves = kNT / 64;
constexpr int kEndNT = 1024;                   // k_pred_end: one workgroup per model (periods, then the snapshot copy)
constexpr int kEndWaves = kEndNT / 64;

DLAP_DEV double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__global__ __launch_bounds__(kNT) void k_pred_loss(PredArgs a) {
  // y, e and dw are single fp32 roundings of the definition: no contraction of R * f into p - y
  // (__fmul_rn is an inlined plain product to this compiler and still fuses). The fp64 products
  // below are exact.
#pragma clang fp contract(off)
  const PredJob& J = a.jobs[blockIdx.y];
  const int2 sg = gp(a.seg)[blockIdx.x];
  const int t = sg.x;
  const int r0 = gp(a.row_ptr)[t] + sg.y;
  const int cnt = min(LINPORT_SEG, gp(a.row_ptr)[t + 1] - r0);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float f = a.f ? gp(a.f)[t] : 1.f;
  const float c2 = 2.f * gp(a.c)[t];                 // (exact)
  const auto pw = gp(J.w);
  const auto pr = gp(a.Rc);
  double s[PRED_NSUM];
#pragma unroll
  for (int k = 0; k < PRED_NSUM; ++k) s[k] = 0.0;
  for (int j = tid; j < cnt; j += kNT) {
    const int row = r0 + j;
    const float p = pw[row], R = pr[row];
    const float y = R * f;                           // one rounding each (contraction is off)
    const float e = p - y;
    if (a.write_dw) gp(J.dw)[row] = c2 * e;
    const double pd = (double)p, ed = (double)e, yd = (double)y;
    s[PRED_SE] += ed * ed;
    s[PRED_SY] += yd * yd;
    s[PRED_S1] += pd;
    s[PRED_SA] += fabs(pd);
    s[PRED_S2] += pd * pd;
    s[PRED_SR] += pd * (double)R;
  }
  __shared__ double red[kWaves][PRED_NSUM];
#pragma unroll
  for (int k = 0; k < PRED_NSUM; ++k) {
    const double x = wave_sum_f64(s[k]);
    if (lane == 0) red[w][k] = x;
  }
  __syncthreads();
  if (tid < PRED_NSUM) {
    double x = red[0][tid];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) x += red[k][tid];
    gp(J.part)[(size_t)blockIdx.x * PRED_NSUM + tid] = x;
  }
}

__global__ __launch_bounds__(kEndNT) void k_pred_end(const PredEndJob* __restrict__ jobs, int smask, int book, int P) {
  const PredEndJob& J = jobs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  __shared__ double red[kEndWaves];
  __shared__ double s_loss[3];
  __shared__ int s_snap;
  for (int sp = 0; sp < 3; ++sp) {
    if (!((smask >> sp) & 1)) {
      if (tid == 0) s_loss[sp] = __builtin_nan("");
      continue;
    }
    const PredSplit& S = J.sp[sp];
    double acc = 0.0;
    for (int t = tid; t < S.T; t += kEndNT) {
      const int s0 = gp(S.seg_ptr)[t], s1 = gp(S.seg_ptr)[t + 1];
      double x[PRED_NSUM];
#pragma unroll
      for (int k = 0; k < PRED_NSUM; ++k) x[k] = 0.0;
      for (int s = s0; s < s1; ++s) {
#pragma unroll
        for (int k = 0; k < PRED_NSUM; ++k) x[k] += gp(S.part)[(size_t)s * PRED_NSUM + k];
      }
#pragma unroll
      for (int k = 0; k < PRED_NSUM; ++k) gp(S.sums)[(size_t)k * S.T + t] = x[k];
      acc += (double)gp(S.c)[t] * x[PRED_SE];
    }
    acc = wave_sum_f64(acc);
    __syncthreads();                                  // (red of the previous split has been read)
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (tid == 0) {
      double x = red[0];
#pragma unroll
      for (int k = 1; k < kEndWaves; ++k) x += red[k];
      s_loss[sp] = x;
      gp(J.loss)[sp] = x;
    }
  }
  if (!book) return;
  if (tid == 0) {
    const int ep = gp(J.ep)[0];
    const float best = gp(J.best)[0];
    const float gn = gp(J.gnorm)[0];
    const bool poisoned = prog_poisoned(J.prog);
    // past the history capacity the row goes to a per-block scratch instead of out of bounds
    __shared__ float spill[PRED_HIST_W];
    float* row = ep < J.max_ep ? J.hist + (size_t)ep * PRED_HIST_W : spill;
    const float nanv = __builtin_nanf("");
    float r[PRED_HIST_W];
    r[PH_TRAIN_LOSS] = poisoned ? nanv : (float)s_loss[0];
    r[PH_VALID_LOSS] = poisoned ? nanv : (float)s_loss[1];
    r[PH_TEST_LOSS] = poisoned ? nanv : (float)s_loss[2];
    r[PH_GNORM] = poisoned ? nanv : gn;
    int up = 0;
    if (!poisoned && ((smask >> 1) & 1) && r[PH_VALID_LOSS] < best) {      // (NaN never wins)
      gp(J.best)[0] = r[PH_VALID_LOSS];
      gp(J.ep)[1] = ep;
      up = 1;
    }
    r[PH_BEST] = (float)up;
#pragma unroll
    for (int c = 0; c < PRED_HIST_W; ++c) row[c] = r[c];
    gp(J.ep)[0] = ep + 1;
    s_snap = up;
  }
  __syncthreads();
  if (s_snap) {
    const auto src = gp(J.params);
    const auto dst = gp(J.snap);
    for (int i = tid; i < P; i += kEndNT) dst[i] = src[i];
  }
}

__global__ __launch_bounds__(64) void k_pred_begin(const PredEndJob* __restrict__ jobs, int njobs) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= njobs) return;
  const PredEndJob& J = jobs[g];
  gp(J.best)[0] = INFINITY;
  gp(J.ep)[0] = 0;
  gp(J.ep)[1] = -1;
}

}  // namespace

void launch_pred_loss(const PredArgs& a, int njobs, hipStream_t st) {
  if (a.nseg <= 0 || njobs <= 0) return;
  if (!a.jobs || !a.Rc || !a.c || !a.row_ptr || !a.seg)
    dlap_throw_hip(hipErrorInvalidValue, "pred_loss: missing arguments", __FILE__, __LINE__);
  hipLaunchKernelGGL(k_pred_loss, dim3((unsigned)a.nseg, (unsigned)njobs), dim3(kNT), 0, st, a);
  HIP_OK(hipGetLastError());
}

void launch_pred_end(const PredEndJob* jobs, int njobs, int smask, int book, int P, hipStream_t st) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(k_pred_end, dim3((unsigned)njobs), dim3(kEndNT), 0, st, jobs, smask, book, P);
  HIP_OK(hipGetLastError());
}

void launch_pred_begin(const PredEndJob* jobs, int njobs, hipStream_t st) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(k_pred_begin, dim3((unsigned)((njobs + 63) / 64)), dim3(64), 0, st, jobs, njobs);
  HIP_OK(hipGetLastError());
}
