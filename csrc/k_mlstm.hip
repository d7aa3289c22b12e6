// The moment network's macro LSTM (paper CSMV; config key `moment_lstm`): forward to the moment
// towers' per-period layer-0 bias table, and phase 2's backward from the table's gradient.
//
//   hm = LSTM(macro)            one layer, width Hm <= 32, PyTorch gate order i, f, g, o, both
//                               biases, zero initial state on every call and split
//   abias[t][c] = W_m0[c, :Hm] . hm_t + b_m0[c]      (c < cm1, zero-padded to 64 columns)
//
// All arithmetic is fp32 in both engine precisions. Kernels order themselves by stream order
// only; every loop is bounded by T, M or Hm; every sum over t runs in a fixed order (no float
// atomics).
//
// Forward
//   k_mlstm_proj  grid (ceil(T/16), ceil(4Hm/16), jobs), one wave per 16x16 tile of
//                 xg[t] = W_ih m_t + b_ih + b_hh on v_mfma_f32_16x16x4_f32, operands straight from
//                 the flat parameters / the macro series (any M, any Hm: edges masked).
//   k_mlstm_rec   one workgroup (4 waves) per job. Wave 0 runs the recurrence with the 4 Hm gate
//                 rows spread over all 64 lanes: with HP = 16 or 32 (Hm padded) and NPART = 64 / HP,
//                 lane l owns unit k = l / NPART and part l % NPART of its gates (one gate at
//                 HP = 16, two at 32), with its rows of W_hh in registers; h is broadcast with
//                 v_readlane, the four activated gates of a unit -- adjacent lanes of one quad --
//                 gathered with quad_perm DPP moves (no LDS round trip on the serial chain), and
//                 every lane keeps (c, h) of its unit. xg streams from global memory eight steps
//                 ahead (any T). Waves 1..3 build the table for the previous 32-period chunk from
//                 the h rows wave 0 left in LDS (two chunk buffers): the table costs one chunk's tail.
// Backward (phase 2, after k_finalize wrote dab)
//   k_mlstm_dhm   grid (ceil(T/8), jobs): dhm[t] = W_m0[:, :Hm]' dab[t], parallel over periods.
//   k_mlstm_bptt  one workgroup per job. Wave 0: BPTT in the forward's lane layout; the gate
//                 gradients of a step are exchanged through LDS, each lane sums its part's rows
//                 of W_hh' d and the parts are added with xor shuffles in a fixed order. Saved
//                 gates / cells / dhm stream from global memory four steps ahead.
//                 Waves 1..3 meanwhile: db_m0 = sum_t dab[t], dW_m0[:, :Hm] = sum_t dab[t] (x) hm[t].
//   k_mlstm_wgrad grid (ceil((M + Hm + 1)/16), jobs): [dW_ih | dW_hh | db] = sum_t dg[t] (x)
//                 [m_t | h_{t-1} | 1] on the matrix cores, the four waves splitting the time
//                 axis and their partial tiles summed in wave order.
#include <algorithm>
#include "common.h"
#include "layout.h"
#include "mlstm.h"

// (the activations of k_rnn.hip, copied: same v_exp + v_rcp forms)
DLAP_DEV float ml_sigm(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
DLAP_DEV float ml_tanh(float x) {
  const float t = 2.f * ml_sigm(2.f * x) - 1.f;
  return fabsf(x) < 0.0125f ? x * (1.f - x * x * (1.f / 3.f)) : t;
}
// sigmoid, or tanh where tnh (branch-free: the gates of a wave differ by lane)
DLAP_DEV float ml_act(float x, bool tnh) {
  const float s = ml_sigm(tnh ? 2.f * x : x);
  const float t = fabsf(x) < 0.0125f ? x * (1.f - x * x * (1.f / 3.f)) : 2.f * s - 1.f;
  return tnh ? t : s;
}
DLAP_DEV float ml_readlane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
// quad_perm DPP: lane l reads lane (l & ~3) + P[l & 3] of its quad (CTRL = P0 | P1 << 2 | P2 << 4 | P3 << 6)
template <int CTRL>
DLAP_DEV float ml_quad(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// ------------------------------------------------------------------ k_mlstm_proj -------
//   A (16x4): lane l -> macro[t = t0 + (l&15)][k = l>>4];  B (4x16): lane l -> W_ih[o = o0 + (l&15)][k = l>>4]
//   C (16x16): lane l -> xg[t0 + 4*(l>>4) + r][o0 + (l&15)]
__global__ __launch_bounds__(64) void k_mlstm_proj(const MlstmJob* __restrict__ jobs,
                                                   const ModelDesc* __restrict__ md) {
  const MlstmJob& J = jobs[blockIdx.z];
  const int T = J.T, M = md->M, G4 = 4 * md->mH;
  const int t0 = blockIdx.x * 16, o0 = blockIdx.y * 16;
  if (t0 >= T || o0 >= G4) return;
  const int l = threadIdx.x, n = l & 15, kq = l >> 4;
  const int ta = min(t0 + n, T - 1), oa = min(o0 + n, G4 - 1);
  const bool ook = o0 + n < G4;
  const auto X = gp(J.macro) + (size_t)ta * M;
  const auto W = gp(J.params) + md->mlstm_w_ih + (size_t)oa * M;
  f32x4 acc = zero4();
  constexpr int KC = 16;
  for (int kb = 0; kb < M; kb += 4 * KC) {
    float a[KC], b[KC];
#pragma unroll
    for (int s = 0; s < KC; ++s) {
      const int m = kb + 4 * s + kq, mc = m < M ? m : 0;
      a[s] = X[mc];
      b[s] = W[mc];
    }
#pragma unroll
    for (int s = 0; s < KC; ++s) {
      const bool ok = kb + 4 * s + kq < M;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? a[s] : 0.f, ok && ook ? b[s] : 0.f, acc, 0, 0, 0);
    }
  }
  const float bias = gp(J.params)[md->mlstm_b_ih + oa] + gp(J.params)[md->mlstm_b_hh + oa];
  if (!ook) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = t0 + 4 * kq + r;
    if (t < T) gp(J.xg)[(size_t)t * G4 + o0 + n] = acc[r] + bias;
  }
}

// ------------------------------------------------------------------- k_mlstm_rec -------
#define MLSTM_TC 32          // periods per LDS chunk of h rows (table epilogue)

template <int HP>
__global__ __launch_bounds__(256) void k_mlstm_rec(const MlstmJob* __restrict__ jobs,
                                                   const ModelDesc* __restrict__ md) {
  constexpr int GPL = HP / 16;               // gates per lane: 1 (HP = 16) or 2 (HP = 32)
  constexpr int NPART = 64 / HP;             // lanes per unit: 4 (one gate each) or 2 (two gates each)
  constexpr int D = 8;                       // xg prefetch distance (steps)
  __shared__ __attribute__((aligned(16))) float s_h[2][MLSTM_TC][HP];
  const MlstmJob& J = jobs[blockIdx.x];
  const int T = J.T, Hm = md->mH, G4 = 4 * Hm;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nch = (T + MLSTM_TC - 1) / MLSTM_TC;
  const auto P = gp(J.params);
  // --- wave 0: recurrence state; the lanes of a unit are adjacent (one quad holds 1 or 2 units),
  // so the unit's four activated gates are gathered with quad_perm DPP moves
  const int k = lane / NPART, part = lane % NPART;
  const bool act = k < Hm;
  float whh[GPL][HP];
  int qg[GPL];
  float c = 0.f, h = 0.f;
  // --- waves 1..3: table state (column cc of period groups tg, tg + 3, ...)
  const int cc = lane, tg = wave - 1;
  const int cm1 = md->cm1;
  const PackLayer& L0 = md->m[0];
  float w0[HP], b0 = 0.f;
  if (wave == 0) {
#pragma unroll
    for (int g = 0; g < GPL; ++g) {
      qg[g] = part * GPL + g;
#pragma unroll
      for (int j = 0; j < HP; ++j) {
        const bool ok = act && j < Hm;
        const float v = P[md->mlstm_w_hh + (qg[g] * Hm + (act ? k : 0)) * Hm + (j < Hm ? j : 0)];
        whh[g][j] = ok ? v : 0.f;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      const bool ok = cc < cm1 && j < Hm;
      const float v = P[L0.w_off + (cc < cm1 ? cc : 0) * L0.ld + (j < Hm ? j : 0)];
      w0[j] = ok ? v : 0.f;
    }
    b0 = cc < cm1 ? P[L0.b_off + cc] : 0.f;
  }
  // (job pointers in registers: the stores of the time loop may alias the job table, so the
  // compiler would reload them every step)
  const auto xg = gp(J.xg);
  const auto sgp = gp(J.sg);
  const auto scp = gp(J.sc);
  const auto hmp = gp(J.hm);
  const auto abp = gp(J.abias);
  const bool save = J.sg != nullptr;
  float cur[D][GPL], nxt[D][GPL];
  auto load = [&](float (&x)[D][GPL], int t0) {
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int g = 0; g < GPL; ++g) {
        const bool ok = act && t0 + d < T;
        const float v = xg[ok ? (size_t)(t0 + d) * G4 + qg[g] * Hm + k : 0];
        x[d][g] = ok ? v : 0.f;
      }
  };
  if (wave == 0) load(cur, 0);
  for (int ch = 0; ch <= nch; ++ch) {
    if (wave == 0 && ch < nch) {
      float (*sh)[HP] = s_h[ch & 1];
      const int tb = ch * MLSTM_TC, te = min(T, tb + MLSTM_TC);
      for (int t0 = tb; t0 < te; t0 += D) {
        load(nxt, t0 + D);
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int t = t0 + d;
          if (t < te) {
            float a[GPL];
#pragma unroll
            for (int g = 0; g < GPL; ++g) a[g] = cur[d][g];
#pragma unroll
            for (int j = 0; j < HP; ++j) {
              const float hj = ml_readlane(h, j * NPART);
#pragma unroll
              for (int g = 0; g < GPL; ++g) a[g] = fmaf(whh[g][j], hj, a[g]);
            }
#pragma unroll
            for (int g = 0; g < GPL; ++g) a[g] = ml_act(a[g], qg[g] == 2);
            float gi, gf, gg, go;
            if constexpr (GPL == 1) {            // quad = (i, f, g, o) of one unit
              gi = ml_quad<0x00>(a[0]); gf = ml_quad<0x55>(a[0]);
              gg = ml_quad<0xAA>(a[0]); go = ml_quad<0xFF>(a[0]);
            } else {                             // quad = ((i, f), (g, o)) of two units
              gi = ml_quad<0xA0>(a[0]); gf = ml_quad<0xA0>(a[1]);
              gg = ml_quad<0xF5>(a[0]); go = ml_quad<0xF5>(a[1]);
            }
            c = gf * c + gi * gg;
            h = go * ml_tanh(c);
            if (act) {
              if (save) {
#pragma unroll
                for (int g = 0; g < GPL; ++g) sgp[(size_t)t * G4 + qg[g] * Hm + k] = a[g];
              }
              if (part == 0) {
                hmp[(size_t)t * Hm + k] = h;
                if (save) scp[(size_t)t * Hm + k] = c;
              }
            }
            if (part == 0) sh[t - tb][k] = h;       // (padded units: 0)
          }
        }
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
          for (int g = 0; g < GPL; ++g) cur[d][g] = nxt[d][g];
      }
    } else if (wave > 0 && ch > 0) {
      const float (*sh)[HP] = s_h[(ch - 1) & 1];
      const int tb = (ch - 1) * MLSTM_TC, te = min(T, tb + MLSTM_TC);
      for (int t = tb + tg; t < te; t += 3) {
        const f32x4* row = reinterpret_cast<const f32x4*>(sh[t - tb]);
        float s = b0;
#pragma unroll
        for (int j4 = 0; j4 < HP / 4; ++j4) {
          const f32x4 v = row[j4];
#pragma unroll
          for (int e = 0; e < 4; ++e) s = fmaf(w0[4 * j4 + e], v[e], s);
        }
        abp[(size_t)t * 64 + cc] = cc < cm1 ? s : 0.f;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------- k_mlstm_dhm -------
// dhm[t][j] = sum_c W_m0[c][j] dab[t][c]; block = 8 periods x 32 units
__global__ __launch_bounds__(256) void k_mlstm_dhm(const MlstmJob* __restrict__ jobs,
                                                   const ModelDesc* __restrict__ md) {
  const MlstmJob& J = jobs[blockIdx.y];
  const int T = J.T, Hm = md->mH, cm1 = md->cm1;
  const int j = threadIdx.x & 31, t = blockIdx.x * 8 + (threadIdx.x >> 5);
  if (t >= T || j >= Hm) return;
  const PackLayer& L0 = md->m[0];
  const auto W = gp(J.params) + L0.w_off + j;
  const auto d = gp(J.dab) + (size_t)t * 64;
  float s = 0.f;
#pragma unroll 8
  for (int c = 0; c < cm1; ++c) s = fmaf(W[(size_t)c * L0.ld], d[c], s);
  gp(J.dhm)[(size_t)t * Hm + j] = s;
}

// ------------------------------------------------------------------ k_mlstm_bptt -------
template <int HP>
__global__ __launch_bounds__(256) void k_mlstm_bptt(const MlstmJob* __restrict__ jobs,
                                                    const ModelDesc* __restrict__ md) {
  constexpr int GPL = HP / 16;
  constexpr int NPART = 64 / HP;
  constexpr int D = 4;
  __shared__ __attribute__((aligned(16))) float s_d[4 * HP];     // [gate q][unit] of the current step
  const MlstmJob& J = jobs[blockIdx.x];
  const int T = J.T, Hm = md->mH, G4 = 4 * Hm;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const auto P = gp(J.params);
  const PackLayer& L0 = md->m[0];
  if (wave > 0) {
    // db_m0 and dW_m0[:, :Hm]: one output per thread and pass, the sum over t in order
    const int cm1 = md->cm1, nout = cm1 * (Hm + 1);
    for (int o = threadIdx.x - 64; o < nout; o += 192) {
      const int c = o / (Hm + 1), j = o - c * (Hm + 1);      // j == Hm: the bias
      const auto d = gp(J.dab) + c;
      const auto hm = gp(J.hm) + (j < Hm ? j : 0);
      float s = 0.f;
#pragma unroll 8
      for (int t = 0; t < T; ++t) s = fmaf(d[(size_t)t * 64], j < Hm ? hm[(size_t)t * Hm] : 1.f, s);
      if (j < Hm) gp(J.grads)[L0.w_off + (size_t)c * L0.ld + j] = s;
      else gp(J.grads)[L0.b_off + c] = s;
    }
    return;
  }
  const int k = lane % HP, part = lane / HP;
  const bool act = k < Hm;
  // rows of W_hh' this lane sums: gate q of its part, every unit j -> Whh[(q Hm + j)][k]
  float wT[GPL][HP];
  int qg[GPL];
#pragma unroll
  for (int g = 0; g < GPL; ++g) {
    qg[g] = part * GPL + g;
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      const bool ok = act && j < Hm;
      const float v = P[md->mlstm_w_hh + (qg[g] * Hm + (j < Hm ? j : 0)) * Hm + (act ? k : 0)];
      wT[g][j] = ok ? v : 0.f;
    }
  }
  const auto sgp = gp(J.sg);
  const auto scp = gp(J.sc);
  const auto dhp = gp(J.dhm);
  const auto dgp = gp(J.dg);
  struct Pre { float gi, gf, gg, go, cp, dh; };
  Pre cur[D], nxt[D];
  // steps run t = T-1 .. 0; slot d of the block starting at t0 is period t0 - d
  auto load = [&](Pre (&x)[D], int t0) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int t = t0 - d;
      const bool ok = act && t >= 0;
      const size_t tg = ok ? (size_t)t : 0;
      const int kk = act ? k : 0;
      const float gi = sgp[tg * G4 + kk], gf = sgp[tg * G4 + Hm + kk];
      const float gg = sgp[tg * G4 + 2 * Hm + kk], go = sgp[tg * G4 + 3 * Hm + kk];
      const float cp = scp[(ok && t > 0 ? (size_t)(t - 1) : 0) * Hm + kk];
      const float dh = dhp[tg * Hm + kk];
      x[d].gi = ok ? gi : 0.f; x[d].gf = ok ? gf : 0.f; x[d].gg = ok ? gg : 0.f; x[d].go = ok ? go : 0.f;
      x[d].cp = ok && t > 0 ? cp : 0.f; x[d].dh = ok ? dh : 0.f;
    }
  };
  load(cur, T - 1);
  float dh_rec = 0.f, dc_next = 0.f;
  for (int t0 = T - 1; t0 >= 0; t0 -= D) {
    load(nxt, t0 - D);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int t = t0 - d;
      if (t >= 0) {
        const Pre& p = cur[d];
        const float cc = p.gf * p.cp + p.gi * p.gg;            // the forward's c_t, same order
        const float tc = ml_tanh(cc);
        const float dh = p.dh + dh_rec;
        const float d_o = dh * tc * p.go * (1.f - p.go);
        const float dc = dh * p.go * (1.f - tc * tc) + dc_next;
        const float d_i = dc * p.gg * p.gi * (1.f - p.gi);
        const float d_f = dc * p.cp * p.gf * (1.f - p.gf);
        const float d_g = dc * p.gi * (1.f - p.gg * p.gg);
        dc_next = dc * p.gf;
        float dq[GPL];
#pragma unroll
        for (int g = 0; g < GPL; ++g) {
          const int q = qg[g];
          dq[g] = q == 0 ? d_i : (q == 1 ? d_f : (q == 2 ? d_g : d_o));
          if (act) dgp[(size_t)t * G4 + q * Hm + k] = dq[g];
          s_d[q * HP + k] = act ? dq[g] : 0.f;
        }
        // one wave: its LDS operations complete in order; the fences keep the compiler from
        // moving the reads over the writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < GPL; ++g) {
          const f32x4* row = reinterpret_cast<const f32x4*>(&s_d[qg[g] * HP]);
#pragma unroll
          for (int j4 = 0; j4 < HP / 4; ++j4) {
            const f32x4 v = row[j4];
#pragma unroll
            for (int e = 0; e < 4; ++e) s = fmaf(wT[g][4 * j4 + e], v[e], s);
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // add the parts in a fixed order (every lane ends with the same total)
        if constexpr (NPART == 4) {
          const float s1 = s + __shfl_xor(s, 16, 64);
          float lo = s1, hi = __shfl_xor(s1, 32, 64);
          if (part >= 2) { const float tmp = lo; lo = hi; hi = tmp; }
          dh_rec = lo + hi;
        } else {
          float lo = s, hi = __shfl_xor(s, 32, 64);
          if (part >= 1) { const float tmp = lo; lo = hi; hi = tmp; }
          dh_rec = lo + hi;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) cur[d] = nxt[d];
  }
}

// ----------------------------------------------------------------- k_mlstm_wgrad -------
//   A lane l -> col value at t = t0 + (l>>4), col = c0 + (l&15);  B lane l -> dg[t][g0 + (l&15)]
//   C lane l -> (col = c0 + 4(l>>4) + r, g = g0 + (l&15))
// columns: [0, M) macro -> dW_ih; [M, M + Hm) h_{t-1} -> dW_hh; M + Hm: ones -> db_ih = db_hh
template <int GT>
__global__ __launch_bounds__(256) void k_mlstm_wgrad(const MlstmJob* __restrict__ jobs,
                                                     const ModelDesc* __restrict__ md) {
  __shared__ f32x4 red[4][GT][64];
  const MlstmJob& J = jobs[blockIdx.y];
  const int T = J.T, M = md->M, Hm = md->mH, G4 = 4 * Hm;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
  const int c0 = blockIdx.x * 16, col = c0 + n;
  const int ta = (T * wave) / 4, tb = (T * (wave + 1)) / 4;
  const auto X = gp(J.macro);
  const auto Hh = gp(J.hm);
  const auto dG = gp(J.dg);
  f32x4 acc[GT];
#pragma unroll
  for (int gt = 0; gt < GT; ++gt) acc[gt] = zero4();
  constexpr int KC = GT >= 8 ? 8 : 16;
  for (int t0 = ta; t0 < tb; t0 += 4 * KC) {
    float a[KC], b[KC][GT];
#pragma unroll
    for (int s = 0; s < KC; ++s) {
      const int t = t0 + 4 * s + kq;
      const bool ok = t < tb;
      const int tc = ok ? t : ta;
      float x;
      if (col < M) x = X[(size_t)tc * M + col];
      else if (col < M + Hm) x = tc > 0 ? Hh[(size_t)(tc - 1) * Hm + (col - M)] : 0.f;
      else x = col == M + Hm ? 1.f : 0.f;
      a[s] = ok ? x : 0.f;
#pragma unroll
      for (int gt = 0; gt < GT; ++gt) {
        const int g = gt * 16 + n;
        const float v = dG[(size_t)tc * G4 + (g < G4 ? g : 0)];
        b[s][gt] = ok && g < G4 ? v : 0.f;
      }
    }
#pragma unroll
    for (int s = 0; s < KC; ++s)
#pragma unroll
      for (int gt = 0; gt < GT; ++gt) acc[gt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s][gt], acc[gt], 0, 0, 0);
  }
#pragma unroll
  for (int gt = 0; gt < GT; ++gt) red[wave][gt][lane] = acc[gt];
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int gt = 0; gt < GT; ++gt) {
    const f32x4 v = red[0][gt][lane] + red[1][gt][lane] + red[2][gt][lane] + red[3][gt][lane];
    const int g = gt * 16 + n;
    if (g >= G4) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cc = c0 + 4 * kq + r;
      if (cc < M) gp(J.grads)[md->mlstm_w_ih + (size_t)g * M + cc] = v[r];
      else if (cc < M + Hm) gp(J.grads)[md->mlstm_w_hh + (size_t)g * Hm + (cc - M)] = v[r];
      else if (cc == M + Hm) {
        gp(J.grads)[md->mlstm_b_ih + g] = v[r];
        gp(J.grads)[md->mlstm_b_hh + g] = v[r];
      }
    }
  }
}

// ------------------------------------------------------------------------ launches -----
static void mlstm_check(const ModelDesc& mh, int tmax) {
  if (mh.mnrnn != 1 || mh.mH < 1 || mh.mH > DLAP_MAX_MH || mh.M < 1 || tmax < 1)
    dlap_throw_hip(hipErrorInvalidValue, "moment LSTM: one layer of width 1..32 and M >= 1", __FILE__, __LINE__);
}

void launch_mlstm_fwd(const MlstmJob* jobs, int njobs, int tmax, const ModelDesc* md, const ModelDesc& mh,
                      hipStream_t st, bool /*train: the jobs carry the save buffers*/) {
  if (njobs <= 0) return;
  mlstm_check(mh, tmax);
  const int G4 = 4 * mh.mH;
  hipLaunchKernelGGL(k_mlstm_proj, dim3((tmax + 15) / 16, (G4 + 15) / 16, njobs), dim3(64), 0, st, jobs, md);
  HIP_OK(hipGetLastError());
  if (mh.mH <= 16) hipLaunchKernelGGL((k_mlstm_rec<16>), dim3(njobs), dim3(256), 0, st, jobs, md);
  else hipLaunchKernelGGL((k_mlstm_rec<32>), dim3(njobs), dim3(256), 0, st, jobs, md);
  HIP_OK(hipGetLastError());
}

void launch_mlstm_bwd(const MlstmJob* jobs, int njobs, int tmax, const ModelDesc* md, const ModelDesc& mh,
                      hipStream_t st) {
  if (njobs <= 0) return;
  mlstm_check(mh, tmax);
  const int G4 = 4 * mh.mH;
  hipLaunchKernelGGL(k_mlstm_dhm, dim3((tmax + 7) / 8, njobs), dim3(256), 0, st, jobs, md);
  HIP_OK(hipGetLastError());
  if (mh.mH <= 16) hipLaunchKernelGGL((k_mlstm_bptt<16>), dim3(njobs), dim3(256), 0, st, jobs, md);
  else hipLaunchKernelGGL((k_mlstm_bptt<32>), dim3(njobs), dim3(256), 0, st, jobs, md);
  HIP_OK(hipGetLastError());
  const dim3 grid((mh.M + mh.mH + 1 + 15) / 16, njobs);
  if (G4 <= 16) hipLaunchKernelGGL((k_mlstm_wgrad<1>), grid, dim3(256), 0, st, jobs, md);
  else if (G4 <= 32) hipLaunchKernelGGL((k_mlstm_wgrad<2>), grid, dim3(256), 0, st, jobs, md);
  else if (G4 <= 64) hipLaunchKernelGGL((k_mlstm_wgrad<4>), grid, dim3(256), 0, st, jobs, md);
  else hipLaunchKernelGGL((k_mlstm_wgrad<8>), grid, dim3(256), 0, st, jobs, md);
  HIP_OK(hipGetLastError());
}
