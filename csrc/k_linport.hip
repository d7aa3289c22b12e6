// Linear benchmark SDFs on the resident panel (linport.h): the characteristic-managed sums and
// the per-period sums of up to 64 linear portfolios per launch.
//
//   k_managed        grid (segments, 64-column blocks), 256 threads. Lane = column, wave = row slot:
//                    a wave reads 64 adjacent columns of one row (128 B of a bf16 row, 256 B of an
//                    fp32 one), thread (wave w, lane) adds rows w, w + 4, .. of the segment in fp64,
//                    the four waves are summed in order through LDS.
//   k_linport        grid (segments), 256 threads, NV = 1, 2 or 4 blocks of 16 candidates. A wave
//                    takes the 16-row tiles w, w + 4, .. of the segment. Per tile the product
//                    [16 rows x F] x [F x 16 NV] runs on v_mfma_f32_16x16x4_f32: rows on the m
//                    axis, candidates on n. The k axis is walked in chunks of 16 columns, lane
//                    group q holding columns 16 c + 4 q + e of its row for the chunk's four k-steps
//                    e (one 8-byte load of a bf16 row, one 16-byte load of an fp32 one); theta sits
//                    in LDS in the matching B-operand order (host-packed, linport_pack_theta), one
//                    ds_read of NV floats per k-step. Columns >= F of a stored row are replaced
//                    by 0 before the product: they may hold anything (0 * NaN would get through a
//                    zero theta). The C layout leaves a lane with rows 4 q + r of candidate
//                    16 v + n: it forms v = fp32(w - c) and adds the four sums in fp64, dead rows
//                    of a ragged last tile contributing nothing (their loads are clamped to the
//                    segment's last row, their terms selected to 0).
//   k_*_reduce       the segment partials of a period, added in index order.
// Reduction order of k_linport: rows r = 0..3 of a tile and the tiles in order within a lane, the
// four lane groups by a fixed xor tree (16, 32), the four waves in order through LDS, the
// segments in order in k_linport_reduce.
// LDS: theta fragments 4 ceil(F / 16) x 64 x NV floats (12 KB at F = 46, NV = 4; 132 KB at F = 512)
// + 8 KB of wave totals.
#include <algorithm>
#include <cstring>
#include "common.h"
#include "linport.h"

namespace {

constexpr int kNT = 256;
constexpr int kWaves = kNT / 64;
constexpr int kMU = 8;                         // k_managed: rows a thread loads before it adds them
constexpr size_t kLdsBudget = 160 * 1024;

__host__ __device__ inline int lp_chunks(int F) { return (F + 15) >> 4; }
__host__ __device__ inline size_t lp_red_bytes(int NV) { return (size_t)kWaves * (4 * NV * 16 + 2) * sizeof(double); }
__host__ __device__ inline size_t lp_lds_bytes(int F, int NV) {
  return (size_t)4 * lp_chunks(F) * 64 * NV * sizeof(float) + lp_red_bytes(NV);
}

template <bool F32>
DLAP_DEV float x_at(const void* X, size_t idx) {
  if constexpr (F32) return gp(reinterpret_cast<const float*>(X))[idx];
  else return __uint_as_float((uint32_t)gp(reinterpret_cast<const u16*>(X))[idx] << 16);
}

template <bool F32>
__global__ __launch_bounds__(kNT) void k_managed(LinportArgs a) {
  const int2 sg = gp(a.seg)[blockIdx.x];
  const int r0 = gp(a.pv.row_ptr)[sg.x] + sg.y;
  const int cnt = min(LINPORT_SEG, gp(a.pv.row_ptr)[sg.x + 1] - r0);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int f = blockIdx.y * 64 + lane;
  const bool live = f < a.pv.F;
  const int col = live ? f : 0;
  double sx = 0.0, sxr = 0.0;
  for (int j0 = w; j0 < cnt; j0 += kWaves * kMU) {
    float x[kMU], r[kMU];
#pragma unroll
    for (int k = 0; k < kMU; ++k) {
      const int j = j0 + k * kWaves;
      const int row = r0 + (j < cnt ? j : 0);        // (clamped: a dead slot re-reads the first row)
      x[k] = x_at<F32>(a.pv.X, (size_t)row * a.pv.KP + col);
      r[k] = gp(a.pv.Rc)[row];
    }
#pragma unroll
    for (int k = 0; k < kMU; ++k) {
      const bool in = live && j0 + k * kWaves < cnt;
      sx += in ? (double)x[k] : 0.0;
      sxr += in ? (double)x[k] * (double)r[k] : 0.0;
    }
  }
  __shared__ double red[kWaves][2][64];
  red[w][0][lane] = sx;
  red[w][1][lane] = sxr;
  __syncthreads();
  if (tid < 128) {
    const int h = tid >> 6;
    double s = red[0][h][lane];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) s += red[k][h][lane];
    if (live) gp(a.part)[((size_t)blockIdx.x * 2 + h) * a.pv.F + f] = s;
  }
}

__global__ __launch_bounds__(kNT) void k_managed_reduce(LinportArgs a) {
  const int i = blockIdx.x * kNT + threadIdx.x;
  if (i >= a.pv.T * a.pv.F) return;
  const int t = i / a.pv.F, f = i - t * a.pv.F;
  const int s0 = gp(a.seg_ptr)[t], s1 = gp(a.seg_ptr)[t + 1];
  double sx = 0.0, sxr = 0.0;
  for (int s = s0; s < s1; ++s) {
    sx += gp(a.part)[((size_t)s * 2) * a.pv.F + f];
    sxr += gp(a.part)[((size_t)s * 2 + 1) * a.pv.F + f];
  }
  gp(a.out)[i] = sx;
  gp(a.out)[(size_t)a.pv.T * a.pv.F + i] = sxr;
  if (f == 0) gp(a.n)[t] = gp(a.pv.row_ptr)[t + 1] - gp(a.pv.row_ptr)[t];
}

// columns 16 c + 4 q .. + 3 of a stored row, the ones >= F replaced by 0
template <bool F32>
DLAP_DEV f32x4 load_chunk(const void* X, size_t rowoff, int col0, int F) {
  f32x4 x;
  if constexpr (F32) {
    x = ld4(gp(reinterpret_cast<const float*>(X)) + rowoff + col0);
  } else {
    const uint2 u = *reinterpret_cast<const DLAP_GLOBAL uint2*>(gp(reinterpret_cast<const u16*>(X)) + rowoff + col0);
    x = f32x4{bf16_lo(u.x), bf16_hi(u.x), bf16_lo(u.y), bf16_hi(u.y)};
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = col0 + e < F ? x[e] : 0.f;
  return x;
}

template <int NV>
DLAP_DEV void lds_theta(const float* p, float (&b)[NV]) {
  if constexpr (NV == 4) {
    const f32x4 v = ld4(p);
    b[0] = v[0]; b[1] = v[1]; b[2] = v[2]; b[3] = v[3];
  } else if constexpr (NV == 2) {
    const f32x2 v = *reinterpret_cast<const f32x2*>(p);
    b[0] = v[0]; b[1] = v[1];
  } else {
    b[0] = p[0];
  }
}

template <bool F32, int NV>
__global__ __launch_bounds__(kNT) void k_linport(LinportArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NC = lp_chunks(a.pv.F), nth = 4 * NC * 64 * NV;
  float* th = reinterpret_cast<float*>(smem);                                  // [4 NC][64][NV]
  double* red = reinterpret_cast<double*>(smem + (size_t)nth * sizeof(float)); // [waves][4 NV 16 + 2]
  constexpr int PW = 4 * NV * 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, n = lane & 15;
  for (int i = 4 * tid; i < nth; i += 4 * kNT)
    *reinterpret_cast<f32x4*>(th + i) = ld4(gp(a.theta) + i);
  const int2 sg = gp(a.seg)[blockIdx.x];
  const int t = sg.x, K = a.K;
  const int r0 = gp(a.pv.row_ptr)[t] + sg.y;
  const int cnt = min(LINPORT_SEG, gp(a.pv.row_ptr)[t + 1] - r0);
  const int ntiles = (cnt + 15) >> 4;
  float c[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) c[v] = a.center && 16 * v + n < K ? gp(a.center)[(size_t)t * K + 16 * v + n] : 0.f;
  double s1[NV], sa[NV], s2[NV], sr[NV], pr = 0.0, prr = 0.0;
#pragma unroll
  for (int v = 0; v < NV; ++v) s1[v] = sa[v] = s2[v] = sr[v] = 0.0;
  __syncthreads();

  for (int tile = w; tile < ntiles; tile += kWaves) {
    const size_t rowoff = (size_t)(r0 + min(tile * 16 + n, cnt - 1)) * a.pv.KP;   // A operand: row n of the tile
    bool ok[4];
    int rowc[4];
    float R[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                              // C layout: rows 4 q + r
      const int j = tile * 16 + 4 * q + r;
      ok[r] = j < cnt;
      rowc[r] = r0 + min(j, cnt - 1);
      R[r] = gp(a.pv.Rc)[rowc[r]];
    }
    f32x4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = zero4();
    f32x4 x = load_chunk<F32>(a.pv.X, rowoff, 4 * q, a.pv.F);
    for (int ch = 0; ch < NC; ++ch) {
      const f32x4 cur = x;
      if (ch + 1 < NC) x = load_chunk<F32>(a.pv.X, rowoff, 16 * (ch + 1) + 4 * q, a.pv.F);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float b[NV];
        lds_theta<NV>(th + ((size_t)(4 * ch + e) * 64 + lane) * NV, b);
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[e], b[v], acc[v], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double Rd = (double)R[r];
      pr += ok[r] ? Rd : 0.0;
      prr += ok[r] ? Rd * Rd : 0.0;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float vf = acc[v][r] - c[v];
        const double vd = (double)vf;
        s1[v] += ok[r] ? vd + (double)c[v] : 0.0;
        sa[v] += ok[r] ? fabs(vd) : 0.0;
        s2[v] += ok[r] ? vd * vd : 0.0;
        sr[v] += ok[r] ? vd * Rd : 0.0;
      }
    }
    if (a.w_out) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!ok[r]) continue;
        const int i = gp(a.pv.rowti)[rowc[r]].y;
#pragma unroll
        for (int v = 0; v < NV; ++v)
          if (16 * v + n < K) gp(a.w_out)[((size_t)(16 * v + n) * a.pv.T + t) * a.pv.N + i] = acc[v][r] - c[v];
      }
    }
  }

  double* rw = red + (size_t)w * (PW + 2);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    double x4[4] = {s1[v], sa[v], s2[v], sr[v]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double x = x4[k];
      x += __shfl_xor(x, 16, 64);
      x += __shfl_xor(x, 32, 64);
      if (q == 0) rw[(k * NV + v) * 16 + n] = x;
    }
  }
  pr += __shfl_xor(pr, 16, 64); pr += __shfl_xor(pr, 32, 64);
  prr += __shfl_xor(prr, 16, 64); prr += __shfl_xor(prr, 32, 64);
  if (lane == 0) { rw[PW] = pr; rw[PW + 1] = prr; }
  __syncthreads();
  for (int i = tid; i < PW + 2; i += kNT) {            // (PW = 256 at NV = 4: two more than the threads)
    double s = red[i];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) s += red[(size_t)k * (PW + 2) + i];
    if (i < PW) gp(a.part)[(size_t)blockIdx.x * PW + i] = s;
    else gp(a.part_r)[(size_t)blockIdx.x * 2 + (i - PW)] = s;
  }
}

template <int NV>
__global__ __launch_bounds__(kNT) void k_linport_reduce(LinportArgs a) {
  constexpr int PW = 4 * NV * 16;
  const int i = blockIdx.x * kNT + threadIdx.x;
  if (i >= a.pv.T * a.K) return;
  const int t = i / a.K, k = i - t * a.K;
  const int s0 = gp(a.seg_ptr)[t], s1 = gp(a.seg_ptr)[t + 1];
  double x[4] = {0.0, 0.0, 0.0, 0.0}, pr = 0.0, prr = 0.0;
  for (int s = s0; s < s1; ++s) {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] += gp(a.part)[(size_t)s * PW + (j * NV + (k >> 4)) * 16 + (k & 15)];
    if (k == 0) { pr += gp(a.part_r)[(size_t)s * 2]; prr += gp(a.part_r)[(size_t)s * 2 + 1]; }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) gp(a.out)[((size_t)j * a.pv.T + t) * a.K + k] = x[j];
  if (k == 0) {
    gp(a.out_r)[t] = pr;
    gp(a.out_r)[a.pv.T + t] = prr;
    gp(a.n)[t] = gp(a.pv.row_ptr)[t + 1] - gp(a.pv.row_ptr)[t];
  }
}

template <bool F32>
void linport_launch_nv(const LinportArgs& a, int NV, hipStream_t st) {
  const dim3 grid((unsigned)a.nseg), block(kNT), rgrid((unsigned)((a.pv.T * a.K + kNT - 1) / kNT));
  const size_t sh = lp_lds_bytes(a.pv.F, NV);
  if (NV == 1) {
    hipLaunchKernelGGL((k_linport<F32, 1>), grid, block, sh, st, a);
    hipLaunchKernelGGL((k_linport_reduce<1>), rgrid, block, 0, st, a);
  } else if (NV == 2) {
    hipLaunchKernelGGL((k_linport<F32, 2>), grid, block, sh, st, a);
    hipLaunchKernelGGL((k_linport_reduce<2>), rgrid, block, 0, st, a);
  } else {
    hipLaunchKernelGGL((k_linport<F32, 4>), grid, block, sh, st, a);
    hipLaunchKernelGGL((k_linport_reduce<4>), rgrid, block, 0, st, a);
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
int linport_nv(int K) { return K <= 16 ? 1 : (K <= 32 ? 2 : 4); }
size_t linport_theta_floats(int F, int K) { return (size_t)4 * lp_chunks(F) * 64 * linport_nv(K); }
bool linport_supported(int F) { return F >= 1 && lp_lds_bytes(F, 4) <= kLdsBudget; }
size_t linport_part_doubles(int nseg, int K) { return (size_t)nseg * 4 * linport_nv(K) * 16; }

int linport_segments(const int* row_ptr, int T, std::vector<int>& seg, std::vector<int>& seg_ptr) {
  seg.clear();
  seg_ptr.assign((size_t)T + 1, 0);
  for (int t = 0; t < T; ++t) {
    for (int off = 0; off < row_ptr[t + 1] - row_ptr[t]; off += LINPORT_SEG) { seg.push_back(t); seg.push_back(off); }
    seg_ptr[t + 1] = (int)(seg.size() / 2);
  }
  return (int)(seg.size() / 2);
}

void linport_pack_theta(const float* theta, int K, int F, float* packed) {
  const int NV = linport_nv(K), NS = 4 * lp_chunks(F);
  for (int s = 0; s < NS; ++s)
    for (int lane = 0; lane < 64; ++lane)
      for (int v = 0; v < NV; ++v) {
        const int k = 16 * v + (lane & 15), col = 16 * (s >> 2) + 4 * (lane >> 4) + (s & 3);
        packed[((size_t)s * 64 + lane) * NV + v] = k < K && col < F ? theta[(size_t)k * F + col] : 0.f;
      }
}

static void linport_check(const LinportArgs& a, const char* what) {
  if (a.pv.F < 1 || a.pv.F > 4096 || a.pv.KP < 16 * lp_chunks(a.pv.F) || a.pv.T < 0 || a.nseg < 0 || a.pv.T > 65535)
    dlap_throw_hip(hipErrorInvalidValue, what, __FILE__, __LINE__);
}

void launch_managed(const LinportArgs& a, hipStream_t st) {
  linport_check(a, "managed: unsupported arguments");
  if (a.pv.T == 0 || a.nseg == 0) return;
  const dim3 grid((unsigned)a.nseg, (unsigned)((a.pv.F + 63) / 64));
  if (a.pv.fp32) hipLaunchKernelGGL((k_managed<true>), grid, dim3(kNT), 0, st, a);
  else hipLaunchKernelGGL((k_managed<false>), grid, dim3(kNT), 0, st, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(k_managed_reduce, dim3((unsigned)((a.pv.T * a.pv.F + kNT - 1) / kNT)), dim3(kNT), 0, st, a);
  HIP_OK(hipGetLastError());
}

void launch_linport(const LinportArgs& a, hipStream_t st) {
  linport_check(a, "linport: unsupported arguments");
  if (a.K < 1 || a.K > LINPORT_MAX_K || !a.theta || !linport_supported(a.pv.F))
    dlap_throw_hip(hipErrorInvalidValue, "linport: unsupported arguments", __FILE__, __LINE__);
  if (a.pv.T == 0 || a.nseg == 0) return;
  const int NV = linport_nv(a.K);
  if (a.pv.fp32) linport_launch_nv<true>(a, NV, st);
  else linport_launch_nv<false>(a, NV, st);
  HIP_OK(hipGetLastError());
}
