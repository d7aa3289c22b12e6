// Per-period characteristic Gram on the resident panel (xgram.h): gram[t] = X_t' X_t over the
// valid rows of period t, with sum R and sum R^2.
//
//   k_xgram   grid (T, ceil(super-tiles / 4)), 256 threads. A workgroup owns one period and four
//             super-tiles, one per wave: feature blocks (2 ia, 2 ia + 1) x (4 ib .. 4 ib + 3) of
//             16 columns, i.e. up to eight 16 x 16 tiles of the Gram, of which the ones with
//             a <= b are computed. It walks the period's rows in steps of 32: the 256 threads stage
//             the rows of the column blocks its waves need (at most 24, listed once in LDS; as
//             many steps at once as the image holds for them, within a run) row-major into an
//             LDS image -- columns >= F and the dead rows of a ragged run selected to 0: they may
//             hold anything -- and per step every wave reads its six operand fragments and
//             issues its MFMAs. The rows are the MFMA k axis, so the operand is
//             the transpose of the stored rows: lane (q, n) holds feature 16 c + n of rows 8 q + j,
//             which is both the A fragment of block c and its B fragment, so one fragment serves
//             every tile of the super-tile it appears in.
//               bf16 panel  v_mfma_f32_16x16x32_bf16, fragments by two ds_read_b64_tr_b16
//                           (rows 8 q .. + 3 and + 4 .. + 7; every lane supplies an in-bounds,
//                           8-byte aligned address: the image is padded, nothing is masked);
//               fp32 panel  eight v_mfma_f32_16x16x4_f32 (k = 8 q + j for MFMA j), fragments by
//                           plain ds_read_b32 of the column.
//             After every XGRAM_RUN rows the fp32 tiles are added to the fp64 accumulators the
//             wave keeps in registers (8 tiles x 4 doubles) and cleared. At the end a lane writes
//             its C-layout elements and their mirror images; of a diagonal tile only i <= j is
//             written, so the lower triangle is a bitwise copy.
//   sum_r, sum_rr (grid.y == 0): thread k adds rows k, k + 256, .. in fp64, a fixed xor tree over
//             the wave, the four waves in order through LDS.
// LDS: 32 x (24 blocks + 16 B pad) = 24.5 KB (bf16) or 48.5 KB (fp32) + the small tables.
#include <algorithm>
#include "common.h"
#include "xgram.h"

namespace {

constexpr int kNT = 256;
constexpr int kWaves = kNT / 64;
constexpr int kSA = 2, kSB = 4;                // feature blocks of a super-tile: rows x columns
constexpr int kFr = kSA + kSB;                 // operand fragments of a wave
constexpr int kSlots = kWaves * kFr;           // column blocks a workgroup stages at most
constexpr int kStep = 32;                      // rows per staged step (the bf16 MFMA's k)

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
#define LDS3 __attribute__((address_space(3)))

template <bool F32> struct XG {
  using P = PrecBF16;
  static constexpr int kBB = 32;               // bytes of one row of a 16-column block
};
template <> struct XG<true> {
  using P = PrecF32;
  static constexpr int kBB = 64;
};
template <bool F32> constexpr int img_max() { return kStep * (kSlots * XG<F32>::kBB + 16); }
template <bool F32> constexpr size_t lds_bytes() {
  return (size_t)img_max<F32>() + 2 * kWaves * sizeof(double) + (2 * kSlots + 4) * sizeof(int);
}

// Fragment of the staged block in `slot`: lane (q, n) <- column n of rows 8 q + j.
template <bool F32>
DLAP_DEV typename XG<F32>::P::Frag frag(const char* img, int stride, int slot, int q, int n) {
  if constexpr (F32) {
    const char* p = img + (8 * q) * stride + slot * 64 + n * 4;
    f32x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = *reinterpret_cast<const float*>(p + j * stride);
    return f;
  } else {
    // transposed read: the lane supplies row 8 q + (n >> 2), columns 4 (n & 3) .. + 3 of the block
    char* p = const_cast<char*>(img) + (8 * q + (n >> 2)) * stride + slot * 32 + (n & 3) * 8;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS3 s16x4*)p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS3 s16x4*)(p + 4 * stride));
    const s16x8 v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  }
}

template <bool F32>
__global__ __launch_bounds__(kNT) void k_xgram(XgramArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using P = typename XG<F32>::P;
  constexpr int BB = XG<F32>::kBB;
  constexpr int CPB = BB / 16;                                  // 16-byte chunks of a block row
  char* img = smem;                                             // [32][stride]
  double* red = reinterpret_cast<double*>(smem + img_max<F32>());          // [2][waves]
  int* tab = reinterpret_cast<int*>(smem + img_max<F32>() + 2 * kWaves * sizeof(double));
  int* s_blk = tab;                                             // [kSlots] staged column blocks
  int* s_slot = tab + kSlots;                                   // [waves][kFr] slot of a wave's fragment
  const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, n = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x, F = a.pv.F, NB = (F + 15) >> 4;
  const int r0 = gp(a.pv.row_ptr)[t], cnt = gp(a.pv.row_ptr)[t + 1] - r0;

  if (tid == 0) {                 // the column blocks of the four super-tiles, each listed once
    int nn = 0;
    for (int v = 0; v < kWaves; ++v) {
      const int st = blockIdx.y * kWaves + v;
      for (int k = 0; k < kFr; ++k) {
        int slot = 0;
        if (st < a.ntiles) {
          const int2 ab = gp(a.tiles)[st];
          const int blk = min(k < kSA ? kSA * ab.x + k : kSB * ab.y + (k - kSA), NB - 1);
          for (slot = 0; slot < nn; ++slot)
            if (s_blk[slot] == blk) break;
          if (slot == nn) s_blk[nn++] = blk;
        }
        s_slot[v * kFr + k] = slot;
      }
    }
    tab[2 * kSlots] = nn;
  }
  __syncthreads();
  const int nneed = tab[2 * kSlots];                            // 1 .. kSlots (0: no super-tile, not launched)
  const int stride = nneed * BB + 16;                           // bytes of an image row
  const int st = blockIdx.y * kWaves + w;
  const bool active = st < a.ntiles;
  int ba[kSA], bb[kSB], sl[kFr];
  {
    const int2 ab = gp(a.tiles)[active ? st : 0];
#pragma unroll
    for (int i = 0; i < kSA; ++i) ba[i] = kSA * ab.x + i;
#pragma unroll
    for (int j = 0; j < kSB; ++j) bb[j] = kSB * ab.y + j;
#pragma unroll
    for (int k = 0; k < kFr; ++k) sl[k] = s_slot[w * kFr + k];
  }
  bool ok[kSA][kSB];
#pragma unroll
  for (int i = 0; i < kSA; ++i)
#pragma unroll
    for (int j = 0; j < kSB; ++j) ok[i][j] = active && ba[i] < NB && bb[j] < NB && ba[i] <= bb[j];

  f32x4 acc[kSA][kSB];
  double sum[kSA][kSB][4];
#pragma unroll
  for (int i = 0; i < kSA; ++i)
#pragma unroll
    for (int j = 0; j < kSB; ++j) {
      acc[i][j] = zero4();
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[i][j][r] = 0.0;
    }

  // rows staged per barrier pair: as many 32-row steps as the image holds for this workgroup's blocks
  // (4 at F = 46, 1 at F = 512); the steps of a run keep their order, so the bits do not depend on it
  const int sps = min(XGRAM_RUN / kStep, img_max<F32>() / (kStep * stride));
  const int srows = sps * kStep, per_row = nneed * CPB;
  for (int run0 = 0; run0 < cnt; run0 += XGRAM_RUN) {
    const int runlen = min(XGRAM_RUN, cnt - run0);
    for (int k0 = 0; k0 < runlen; k0 += srows) {
      const int nsub = min(sps, (runlen - k0 + kStep - 1) / kStep), nchunk = nsub * kStep * per_row;
      __syncthreads();                                          // (the previous stage's reads are done)
      for (int c = tid; c < nchunk; c += kNT) {
        const int row = c / per_row, rem = c - row * per_row;
        const int j = rem / CPB, h = rem - j * CPB;
        const int col0 = s_blk[j] * 16 + h * (F32 ? 4 : 8);
        const bool live = k0 + row < runlen;
        const size_t src = (size_t)(r0 + run0 + (live ? k0 + row : 0)) * a.pv.KP + col0;   // (a dead row re-reads a live one)
        u32x4 v;
        if constexpr (F32) {
          v = *reinterpret_cast<const DLAP_GLOBAL u32x4*>(gp(reinterpret_cast<const float*>(a.pv.X)) + src);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = live && col0 + e < F ? v[e] : 0u;
        } else {
          v = *reinterpret_cast<const DLAP_GLOBAL u32x4*>(gp(reinterpret_cast<const u16*>(a.pv.X)) + src);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t m = (live && col0 + 2 * e < F ? 0xFFFFu : 0u) | (live && col0 + 2 * e + 1 < F ? 0xFFFF0000u : 0u);
            v[e] &= m;
          }
        }
        *reinterpret_cast<u32x4*>(img + row * stride + j * BB + h * 16) = v;
      }
      __syncthreads();
      if (active) {
        for (int sub = 0; sub < nsub; ++sub) {
          const char* im = img + sub * kStep * stride;
          typename P::Frag fa[kSA], fb[kSB];
#pragma unroll
          for (int i = 0; i < kSA; ++i) fa[i] = frag<F32>(im, stride, sl[i], q, n);
#pragma unroll
          for (int j = 0; j < kSB; ++j) fb[j] = frag<F32>(im, stride, sl[kSA + j], q, n);
#pragma unroll
          for (int i = 0; i < kSA; ++i)
#pragma unroll
            for (int j = 0; j < kSB; ++j)
              if (ok[i][j]) acc[i][j] = P::mma(fa[i], fb[j], acc[i][j]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kSA; ++i)                               // the run's fp32 Gram joins the fp64 sums
#pragma unroll
      for (int j = 0; j < kSB; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[i][j][r] += (double)acc[i][j][r];
        acc[i][j] = zero4();
      }
  }

  DLAP_GLOBAL double* G = gp(a.gram) + (size_t)t * F * F;
#pragma unroll
  for (int i = 0; i < kSA; ++i)
#pragma unroll
    for (int j = 0; j < kSB; ++j) {
      if (!ok[i][j]) continue;
      const int gj = 16 * bb[j] + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {                             // C layout: rows 4 q + r, column n
        const int gi = 16 * ba[i] + 4 * q + r;
        if (gi >= F || gj >= F || gi > gj) continue;            // (gi > gj: a diagonal tile's lower half)
        G[(size_t)gi * F + gj] = sum[i][j][r];
        if (gi != gj) G[(size_t)gj * F + gi] = sum[i][j][r];
      }
    }

  if (blockIdx.y == 0) {
    double pr = 0.0, prr = 0.0;
    for (int j = tid; j < cnt; j += kNT) {
      const double R = (double)gp(a.pv.Rc)[r0 + j];
      pr += R;
      prr += R * R;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      pr += __shfl_xor(pr, o, 64);
      prr += __shfl_xor(prr, o, 64);
    }
    if (lane == 0) { red[w] = pr; red[kWaves + w] = prr; }
    __syncthreads();
    if (tid < 2) {
      double s = red[tid * kWaves];
#pragma unroll
      for (int k = 1; k < kWaves; ++k) s += red[tid * kWaves + k];
      gp(a.sum_r)[(size_t)tid * a.pv.T + t] = s;
    }
    if (tid == 2) gp(a.n)[t] = cnt;
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
int xgram_run() { return XGRAM_RUN; }

void xgram_tiles(int F, std::vector<int>& tiles) {
  const int NB = (F + 15) / 16, na = (NB + kSA - 1) / kSA, nb = (NB + kSB - 1) / kSB;
  tiles.clear();
  for (int ib = 0; ib < nb; ++ib)
    for (int ia = 0; ia < na; ++ia)
      if (kSA * ia <= std::min(kSB * ib + kSB - 1, NB - 1)) { tiles.push_back(ia); tiles.push_back(ib); }
}

void launch_xgram(const XgramArgs& a, hipStream_t st) {
  const int NB = (a.pv.F + 15) / 16;
  if (a.pv.F < 1 || a.pv.F > 4096 || a.pv.KP < 16 * NB || a.pv.KP % 16 != 0 || a.pv.T < 0 || a.pv.T > 65535 || a.ntiles < 1 || !a.tiles)
    dlap_throw_hip(hipErrorInvalidValue, "xgram: unsupported arguments", __FILE__, __LINE__);
  if (a.pv.T == 0) return;
  const dim3 grid((unsigned)a.pv.T, (unsigned)((a.ntiles + kWaves - 1) / kWaves));
  if (a.pv.fp32) hipLaunchKernelGGL((k_xgram<true>), grid, dim3(kNT), lds_bytes<true>(), st, a);
  else hipLaunchKernelGGL((k_xgram<false>), grid, dim3(kNT), lds_bytes<false>(), st, a);
  HIP_OK(hipGetLastError());
}
