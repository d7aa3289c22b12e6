// Cross-sectional rank transform of a raw characteristic panel (xrank.h).
//
//   k_xrank   grid (ceil(F / CB), periods), 64 .. 1024 threads. A workgroup owns one period and a
//             block of CB = 1, 2, 4 or 8 adjacent columns; with P = N rounded up to a power of two
//             (>= 8) its LDS holds the CB columns side by side, [CB][P] uint32 keys (+ CB counts).
//             1. Keys: the rows are read as CB consecutive floats; a participant's key is
//                qkey_u32(x), everything else (missing, dead row, row >= N, column >= F) is the pad
//                0xFFFFFFFF, which no participant maps to (it is the key of a NaN).
//             2. Bitonic sort of all CB P keys at once, ascending in every column (the direction of
//                a compare-exchange is taken from the index inside the column). A thread sorts 8
//                consecutive keys in registers (stages 2, 4, 8 and the steps 4, 2, 1 of every later
//                stage: two ds_read_b128, two ds_write_b128); the steps >= 8 go two at a time, a
//                thread holding the four keys b, b + q, b + 2q, b + 3q (steps 2q then q), with one
//                single step when their number is odd. log2 P = 12: 35 passes over the keys for 78 steps.
//             3. m = lower bound of the pad in the sorted column -> cnt.
//             4. Every element is read again by the thread that writes it: lt = lower bound of its
//                key among the m sorted keys, lt + eq = upper bound (galloping from lt, so a
//                distinct key costs one probe), out = float(2 lt + eq - m) / float(2 m).
//             The launcher sizes CB and the workgroup by N: CB P <= 8192 keys (32 KiB, four
//             workgroups of 512 threads on a CU at N = 3000), one column and 1024 threads above that.
// Every loop is bounded by N, CB or log2 N.
#include <algorithm>
#include "common.h"
#include "qsort_dev.h"
#include "xrank.h"

namespace {

constexpr uint32_t kPad = 0xFFFFFFFFu;
constexpr int kMaxCB = 8;                      // columns of a workgroup at most
constexpr int kBlockKeys = XRANK_BLOCK_KEYS;   // keys of a workgroup while more than one column fits

struct XrankArgs {
  const float* x;           // [periods][N][F]
  const uint8_t* rowok;     // [periods][N]
  float* out;               // [periods][N][F] (may be x)
  int* cnt;                 // [periods][F]
  int N, F;
  int lp, lcb;              // log2 P, log2 CB
  float thr, fill_missing, fill_dead;
};

DLAP_DEV void cex(uint32_t& a, uint32_t& b, bool up) {
  const uint32_t lo = min(a, b), hi = max(a, b);
  a = up ? lo : hi;
  b = up ? hi : lo;
}

// Steps J0, J0 / 2, .., 1 on 8 consecutive keys. K = 2, 4: the stage, whose direction changes inside
// the 8 keys; K = 0: one direction for all of them.
template <int J0, int K>
DLAP_DEV void local_steps(uint32_t (&v)[8], bool up) {
#pragma unroll
  for (int j = J0; j >= 1; j >>= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (!(e & j)) cex(v[e], v[e | j], K ? !(e & K) : up);
}

DLAP_DEV void load8(const uint32_t* p, uint32_t (&v)[8]) {
  const u32x4 a = *reinterpret_cast<const u32x4*>(p), b = *reinterpret_cast<const u32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
DLAP_DEV void store8(uint32_t* p, const uint32_t (&v)[8]) {
  *reinterpret_cast<u32x4*>(p) = u32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<u32x4*>(p + 4) = u32x4{v[4], v[5], v[6], v[7]};
}

// first index in [lo, lo + n) whose key is >= key (STRICT) or > key (!STRICT), else lo + n
template <bool STRICT>
DLAP_DEV int bound(const uint32_t* col, int lo, int n, uint32_t key) {
  while (n > 0) {
    const int h = n >> 1;
    const uint32_t v = col[lo + h];
    const bool right = STRICT ? v < key : v <= key;
    lo = right ? lo + h + 1 : lo;
    n = right ? n - h - 1 : h;
  }
  return lo;
}

__global__ __launch_bounds__(1024) void k_xrank(XrankArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s[];   // [CB][P] keys, [CB] counts
  const int tid = threadIdx.x, nt = blockDim.x;
  const int N = a.N, F = a.F, lp = a.lp, lcb = a.lcb;
  const int P = 1 << lp, CB = 1 << lcb, tot = CB << lp;
  const int c0 = blockIdx.x << lcb;
  const size_t row0 = (size_t)blockIdx.y * N;
  const DLAP_GLOBAL float* x = gp(a.x) + row0 * F;
  DLAP_GLOBAL float* out = gp(a.out) + row0 * F;
  const DLAP_GLOBAL uint8_t* ok = gp(a.rowok) + row0;

  // 1. keys
  for (int g = tid; g < tot; g += nt) {
    const int row = g >> lcb, c = g & (CB - 1);
    uint32_t key = kPad;
    if (row < N && c0 + c < F && ok[row]) {
      const float v = x[(size_t)row * F + c0 + c];
      if (v > a.thr) key = qkey_u32(v);
    }
    s[(c << lp) + row] = key;
  }
  __syncthreads();

  // 2. sort. Stages 2, 4, 8 in registers
  const int n8 = tot >> 3;
  for (int it = tid; it < n8; it += nt) {
    uint32_t v[8];
    load8(s + 8 * it, v);
    local_steps<1, 2>(v, true);
    local_steps<2, 4>(v, true);
    local_steps<4, 0>(v, (((8 * it) & (P - 1)) & 8) == 0);
    store8(s + 8 * it, v);
  }
  for (int lk = 4; lk <= lp; ++lk) {            // stage k = 2^lk: steps k / 2 .. 8 in LDS, 4 2 1 in registers
    const int k = 1 << lk;
    int lj = lk - 1;
    if ((lj - 2) & 1) {                         // an odd number of steps >= 8: one on its own
      __syncthreads();
      const int j = 1 << lj;
      for (int it = tid; it < (tot >> 1); it += nt) {
        const int i = ((it >> lj) << (lj + 1)) | (it & (j - 1));
        uint32_t e0 = s[i], e1 = s[i + j];
        cex(e0, e1, ((i & (P - 1)) & k) == 0);
        s[i] = e0;
        s[i + j] = e1;
      }
      --lj;
    }
    for (; lj >= 4; lj -= 2) {                  // steps 2 q and q on the keys b, b + q, b + 2 q, b + 3 q
      __syncthreads();
      const int lq = lj - 1, q = 1 << lq;
      for (int it = tid; it < (tot >> 2); it += nt) {
        const int b = ((it >> lq) << (lq + 2)) | (it & (q - 1));
        const bool up = ((b & (P - 1)) & k) == 0;
        uint32_t e0 = s[b], e1 = s[b + q], e2 = s[b + 2 * q], e3 = s[b + 3 * q];
        cex(e0, e2, up);
        cex(e1, e3, up);
        cex(e0, e1, up);
        cex(e2, e3, up);
        s[b] = e0;
        s[b + q] = e1;
        s[b + 2 * q] = e2;
        s[b + 3 * q] = e3;
      }
    }
    __syncthreads();
    for (int it = tid; it < n8; it += nt) {
      uint32_t v[8];
      load8(s + 8 * it, v);
      local_steps<4, 0>(v, (((8 * it) & (P - 1)) & k) == 0);
      store8(s + 8 * it, v);
    }
  }
  __syncthreads();

  // 3. participants per column
  if (tid < CB) {
    const int m = bound<true>(s + (tid << lp), 0, P, kPad);
    s[tot + tid] = (uint32_t)m;
    if (c0 + tid < F) gp(a.cnt)[(size_t)blockIdx.y * F + c0 + tid] = m;
  }
  __syncthreads();

  // 4. ranks
  for (int g = tid; g < (N << lcb); g += nt) {
    const int row = g >> lcb, c = g & (CB - 1);
    if (c0 + c >= F) continue;
    const size_t idx = (size_t)row * F + c0 + c;
    float y = a.fill_dead;
    if (ok[row]) {
      y = a.fill_missing;
      const float v = x[idx];
      if (v > a.thr) {
        const uint32_t key = qkey_u32(v);
        const uint32_t* col = s + (c << lp);
        const int m = (int)s[tot + c];
        const int lt = bound<true>(col, 0, m, key);             // col[lt] == key: the element itself is there
        int w = 1;
        while (lt + w < m && col[lt + w] == key) w <<= 1;       // col[lt + w / 2] == key, col[lt + w] > key or past the end
        const int lo = lt + (w >> 1) + 1;
        const int le = bound<false>(col, lo, min(lt + w, m) - lo, key);   // lt + eq
        y = (float)(lt + le - m) / (float)(2 * m);
      }
    }
    out[idx] = y;
  }
}

int ceil_log2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
int xrank_block_keys() { return kBlockKeys; }

void launch_xrank(const float* x, const uint8_t* rowok, float* out, int* cnt, long long T, int N, int F,
                  float thr, float fill_missing, float fill_dead, hipStream_t st) {
  if (!xrank_supported(N) || F < 1 || T < 0 || !x || !rowok || !out || !cnt)
    dlap_throw_hip(hipErrorInvalidValue, "xrank: unsupported arguments", __FILE__, __LINE__);
  XrankArgs a{};
  a.N = N; a.F = F; a.thr = thr; a.fill_missing = fill_missing; a.fill_dead = fill_dead;
  a.lp = std::max(3, ceil_log2(N));
  a.lcb = 0;
  while ((2 << a.lcb) <= kMaxCB && (2 << a.lcb) <= (1 << ceil_log2(F)) && ((2 << a.lcb) << a.lp) <= kBlockKeys) ++a.lcb;
  const int tot = (1 << a.lcb) << a.lp;                          // 8 .. 32768 keys
  const int nt = std::min(1024, std::max(64, (tot / 16 + 63) / 64 * 64));
  const size_t lds = ((size_t)tot + (1u << a.lcb)) * sizeof(uint32_t);
  if (lds > 64 * 1024) {                                         // (idempotent; more than the default limit)
    static bool raised = false;
    if (!raised) {
      HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_xrank), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      raised = true;
    }
  }
  const unsigned gx = (unsigned)((F + (1 << a.lcb) - 1) >> a.lcb);
  for (long long t0 = 0; t0 < T; t0 += 65535) {
    const long long tc = std::min<long long>(65535, T - t0);
    a.x = x + (size_t)t0 * N * F;
    a.out = out + (size_t)t0 * N * F;
    a.rowok = rowok + (size_t)t0 * N;
    a.cnt = cnt + (size_t)t0 * F;
    hipLaunchKernelGGL(k_xrank, dim3(gx, (unsigned)tc), dim3(nt), lds, st, a);
    HIP_OK(hipGetLastError());
  }
}
