// Batched elastic-net coordinate descent along penalty paths (encd.h).
//
//   k_encd<EPT, PRE>   grid (paths), ENCD_THREADS threads: one workgroup per path. LDS: th, b, the
//             diagonal of M ([n] fp64 each), g (padded to a whole number of elements per thread), the row
//             hints succ [n] int32 and a few words per wave.
//             A step finds the next coordinate that changes and applies it:
//             1. Scan. Thread t looks at the coordinates base + t, base = NT floor(j0 / NT), + NT, ..:
//                a zero coordinate with |rho| <= l1 stays zero without a division, anything else gets
//                the full soft threshold and d. One ballot per wave and base; a wave stops at its
//                first base with a set bit (its lowest j), its lane leaves d and new in the wave's
//                slot, and after one barrier every thread takes the lowest j of the NT / 64 slots in
//                slot order.
//             2. Update. Column j of the symmetric M is row j: g[i] += M[j][i] d, coalesced;
//                th[j] = new; j0 = j + 1; one barrier.
//             3. No coordinate left: the sweep ends (max |th| and the count of non-zeros by a wave
//                shuffle and the slots), and with it possibly the point, the path or the launch.
//             A sweep costs (updates + 1) scans instead of n serial steps.
//             Rows (PRE): a thread holds its EPT = ceil(n / NT) (rounded up to a power of two, <= 32)
//             elements of a row in registers. succ[j] is the coordinate that was updated after j the
//             last time; its row is requested before the update with row j starts, so in a settled
//             active set every row but the first is in flight while the previous update and the scan
//             run. A wrong hint costs a reload, never a bit: the tag of the row in flight is compared
//             with the j the scan found. Past EPT = 32 (or with ENCD_PREFETCH = 0) the update reads
//             its row where it needs it.
// Every loop is bounded by n, n1 max_sweeps or sweeps_per_launch.
#include <algorithm>
#include <climits>
#include "common.h"
#include "encd.h"

namespace {

constexpr int kNT = ENCD_THREADS;
constexpr int kNW = kNT / 64;
constexpr int kMaxEpt = 32;               // row elements of a thread held in registers, at most
constexpr double kTol = 1e-10;

struct EncdArgs {
  const double* A;          // [NA][n][n]
  const int* a_of;          // [P]
  const double* b;          // [P][n]
  const double* l1s;        // [P][n1]
  const double* l2;         // [P]
  double* theta;            // [P][n1][n]
  int* sweeps;              // [P][n1]
  int* nnz;                 // [P][n1]
  double* st_d;             // [P][2][n]
  int* st_i;                // [P][4]
  int n, n1, max_sweeps, max_assets, spl;
};

struct Ctx {
  double *th, *g, *bb, *mjj, *sl_d, *sl_new, *red_mx;
  int *sl_j, *red_cnt, *succ;
  const DLAP_GLOBAL double* M;
  const DLAP_GLOBAL double* l1s;
  DLAP_GLOBAL double* theta;
  DLAP_GLOBAL int* sweeps;
  DLAP_GLOBAL int* nnz;
  double l1, l2, step;
  int n, n1, max_sweeps, max_assets;
  int left;                 // sweeps left in this launch
  int k, sw, j0, jprev, done;
  int upd;                  // updates of the path so far (saturating; a statistic, no output depends on it)
};

// Workgroup-uniform values as scalars. Everything that steers the control flow is uniform, but comes
// out of LDS or global memory, which the compiler has to take for divergent: it would then join the
// paths of the step loop in flow blocks and wait for every row in flight at the joins. (For a load the
// wait also happens here, not where the scan first reads the value.)
DLAP_DEV int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
DLAP_DEV double uniform_f64(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// The next coordinate whose value changes, with its d and new value; false when the launch ends
// (path done or the launch's sweeps used up). Uniform over the workgroup.
DLAP_DEV bool next_update(Ctx& c, int& j, double& d, double& nw) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = c.n;
  for (;;) {
    int cand = INT_MAX;
    for (int base = (c.j0 / kNT) * kNT; base < n; base += kNT) {
      const int i = base + tid;
      bool nz = false;
      double dd = 0.0, nn = 0.0;
      if (i >= c.j0 && i < n) {
        const double t = c.th[i], m = c.mjj[i];
        const double rho = c.bb[i] - (c.g[i] - m * t);
        const double ar = fabs(rho);
        if (!(t == 0.0 && ar <= c.l1)) {        // (else new = +-0 and d = 0)
          const double dg = m + c.l2;
          if (dg > 0.0) {
            double s = ar - c.l1;
            s = s <= 0.0 ? 0.0 : s;
            nn = copysign(s, rho) / dg;
          }
          dd = nn - t;
          nz = dd != 0.0;
        }
      }
      const unsigned long long bal = __ballot(nz);
      if (bal) {
        const int src = __ffsll(bal) - 1;
        cand = base + (wave << 6) + src;
        if (lane == src) { c.sl_d[wave] = dd; c.sl_new[wave] = nn; }
        break;
      }
    }
    if (lane == 0) c.sl_j[wave] = cand;
    __syncthreads();
    int best = INT_MAX, bw = 0;
#pragma unroll
    for (int w = 0; w < kNW; ++w) {
      const int v = c.sl_j[w];
      if (v < best) { best = v; bw = w; }
    }
    best = uniform_i32(best);
    if (best != INT_MAX) {
      bw = uniform_i32(bw);
      j = best; d = uniform_f64(c.sl_d[bw]); nw = uniform_f64(c.sl_new[bw]);
      return true;
    }
    // the sweep is over
    double mx = 0.0;
    int cnt = 0;
    for (int i = tid; i < n; i += kNT) {
      const double t = c.th[i];
      mx = fmax(mx, fabs(t));
      cnt += t != 0.0 ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mx = fmax(mx, __shfl_xor(mx, o, 64));
      cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) { c.red_mx[wave] = mx; c.red_cnt[wave] = cnt; }
    __syncthreads();
    mx = 0.0; cnt = 0;
#pragma unroll
    for (int w = 0; w < kNW; ++w) { mx = fmax(mx, c.red_mx[w]); cnt += c.red_cnt[w]; }
    mx = uniform_f64(mx); cnt = uniform_i32(cnt);
    ++c.sw; --c.left;
    const bool conv = c.step <= kTol * fmax(1.0, mx);
    c.step = 0.0; c.j0 = 0;
    if (conv || c.sw >= c.max_sweeps) {          // the point is over
      DLAP_GLOBAL double* out = c.theta + (size_t)c.k * n;
      for (int i = tid; i < n; i += kNT) out[i] = c.th[i];
      if (tid == 0) { c.sweeps[c.k] = c.sw; c.nnz[c.k] = cnt; }
      ++c.k; c.sw = 0;
      if (c.k >= c.n1 || (c.max_assets >= 0 && cnt > c.max_assets)) { c.done = 1; return false; }
      c.l1 = uniform_f64(c.l1s[c.k]);
    }
    if (c.left <= 0) return false;
  }
}

template <int EPT>
DLAP_DEV void load_row(const Ctx& c, double (&r)[EPT], int j) {
  const DLAP_GLOBAL double* row = c.M + (size_t)j * c.n;
#pragma unroll
  for (int e = 0; e < EPT; ++e) r[e] = row[min(e * kNT + (int)threadIdx.x, c.n - 1)];   // (clamped: always in the row)
}

DLAP_DEV void finish_update(Ctx& c, int j, double d, double nw) {
  if (threadIdx.x == 0) {
    c.th[j] = nw;
    if (c.jprev >= 0 && c.jprev != j) c.succ[c.jprev] = j;
  }
  c.jprev = j;
  c.upd += c.upd < INT_MAX ? 1 : 0;
  c.step = fmax(c.step, fabs(d));
  c.j0 = j + 1;
  __syncthreads();
}

// The update loop with the hinted next row in flight: nxt holds (or is being sent) row tnxt. One
// static copy of the scan, and nxt live across it, so that the compiler neither reuses the registers
// of a row in flight nor waits for it before the update that needs it.
template <int EPT>
DLAP_DEV void run_pre(Ctx& c) {
  double nxt[EPT], prod[EPT];
  int tnxt = -1, j;
  double d, nw;
  while (next_update(c, j, d, nw)) {
    if (j != tnxt) load_row<EPT>(c, nxt, j);     // a wrong hint or none
#pragma unroll
    for (int e = 0; e < EPT; ++e) prod[e] = nxt[e] * d;   // (the row's registers are free for the next one)
    const int pj = uniform_i32(c.succ[j]);
    tnxt = pj < 0 ? j : pj;
    load_row<EPT>(c, nxt, tnxt);                 // requested before the update, used after the next scan
#pragma unroll
    for (int e = 0; e < EPT; ++e) {              // (no branch: g is padded to EPT kNT elements, the pad is never read)
      const int i = e * kNT + (int)threadIdx.x;
      c.g[i] = c.g[i] + prod[e];
    }
    finish_update(c, j, d, nw);
  }
}

DLAP_DEV bool step_plain(Ctx& c) {
  int j;
  double d, nw;
  if (!next_update(c, j, d, nw)) return false;
  const DLAP_GLOBAL double* row = c.M + (size_t)j * c.n;
  for (int i = threadIdx.x; i < c.n; i += kNT) c.g[i] = c.g[i] + row[i] * d;
  finish_update(c, j, d, nw);
  return true;
}

template <int EPT, bool PRE>
__global__ __launch_bounds__(kNT) void k_encd(EncdArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = a.n, tid = threadIdx.x;
  const size_t p = blockIdx.x;
  DLAP_GLOBAL int* sti = gp(a.st_i) + 4 * p;
  if (uniform_i32(sti[2])) return;               // done in an earlier launch
  Ctx c;
  const int npad = PRE ? EPT * kNT : n;          // g: a whole number of elements per thread (run_pre)
  c.th = sm; c.bb = sm + n; c.mjj = sm + 2 * (size_t)n; c.g = sm + 3 * (size_t)n;
  c.sl_d = c.g + npad; c.sl_new = c.sl_d + kNW; c.red_mx = c.sl_new + kNW;
  c.sl_j = reinterpret_cast<int*>(c.red_mx + kNW); c.red_cnt = c.sl_j + kNW; c.succ = c.red_cnt + kNW;
  c.M = gp(a.A) + (size_t)gp(a.a_of)[p] * n * n;
  c.l1s = gp(a.l1s) + p * a.n1;
  c.theta = gp(a.theta) + p * a.n1 * n;
  c.sweeps = gp(a.sweeps) + p * a.n1;
  c.nnz = gp(a.nnz) + p * a.n1;
  c.n = n; c.n1 = a.n1; c.max_sweeps = a.max_sweeps; c.max_assets = a.max_assets; c.left = a.spl;
  c.k = uniform_i32(sti[0]); c.sw = uniform_i32(sti[1]); c.upd = uniform_i32(sti[3]); c.done = 0; c.j0 = 0; c.jprev = -1; c.step = 0.0;
  c.l2 = uniform_f64(gp(a.l2)[p]);
  c.l1 = uniform_f64(c.l1s[c.k]);
  DLAP_GLOBAL double* std_ = gp(a.st_d) + p * 2 * n;
  const DLAP_GLOBAL double* b = gp(a.b) + p * n;
  for (int i = tid; i < n; i += kNT) {
    c.th[i] = std_[i];
    c.g[i] = std_[n + i];
    c.bb[i] = b[i];
    c.mjj[i] = c.M[(size_t)i * n + i];
    c.succ[i] = -1;
  }
  for (int i = n + tid; i < npad; i += kNT) c.g[i] = 0.0;
  __syncthreads();

  if constexpr (PRE) {
    run_pre<EPT>(c);
  } else {
    while (step_plain(c)) {}
  }

  // (th and g are final: the last barrier of next_update is behind every write)
  for (int i = tid; i < n; i += kNT) {
    std_[i] = c.th[i];
    std_[n + i] = c.g[i];
  }
  if (tid == 0) { sti[0] = c.k; sti[1] = c.sw; sti[2] = c.done; sti[3] = c.upd; }
}

size_t lds_bytes(int n, int npad) {
  return ((size_t)3 * n + npad + 3 * kNW) * sizeof(double) + ((size_t)n + 2 * kNW) * sizeof(int);
}

template <int EPT, bool PRE>
void launch_one(const EncdArgs& a, long long P, hipStream_t st) {
  const size_t lds = lds_bytes(a.n, PRE ? EPT * kNT : a.n);      // at most 36 ENCD_MAX_N + 32 kNW bytes
  if (lds > 64 * 1024) {                                         // (idempotent; more than the default limit)
    static bool raised = false;
    if (!raised) {
      HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_encd<EPT, PRE>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      raised = true;
    }
  }
  hipLaunchKernelGGL((k_encd<EPT, PRE>), dim3((unsigned)P), dim3(kNT), lds, st, a);
  HIP_OK(hipGetLastError());
}

void launch(const EncdArgs& a, long long P, hipStream_t st) {
  const int ept = (a.n + kNT - 1) / kNT;
  if (!ENCD_PREFETCH || ept > kMaxEpt) launch_one<1, false>(a, P, st);
  else if (ept <= 1) launch_one<1, true>(a, P, st);
  else if (ept <= 2) launch_one<2, true>(a, P, st);
  else if (ept <= 4) launch_one<4, true>(a, P, st);
  else if (ept <= 8) launch_one<8, true>(a, P, st);
  else if (ept <= 16) launch_one<16, true>(a, P, st);
  else launch_one<32, true>(a, P, st);
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
int encd_threads() { return kNT; }
int encd_prefetch() { return ENCD_PREFETCH; }

int encd_run(const double* A, const int* a_of, const double* b, const double* l1s, const double* l2, double* theta,
             int* sweeps, int* nnz, void* state, int NA, long long P, int n, int n1, int max_sweeps, int max_assets,
             int sweeps_per_launch, hipStream_t st, std::vector<float>* ms, std::vector<int>* updates) {
  if (!encd_supported(n) || NA < 1 || P < 1 || P > 0x7FFFFFFFll || n1 < 1 || max_sweeps < 1 || sweeps_per_launch < 1 ||
      !A || !a_of || !b || !l1s || !l2 || !theta || !sweeps || !nnz || !state)
    dlap_throw_hip(hipErrorInvalidValue, "en_paths: unsupported arguments", __FILE__, __LINE__);
  EncdArgs a{};
  a.A = A; a.a_of = a_of; a.b = b; a.l1s = l1s; a.l2 = l2; a.theta = theta; a.sweeps = sweeps; a.nnz = nnz;
  a.st_d = static_cast<double*>(state);
  a.st_i = reinterpret_cast<int*>(a.st_d + (size_t)P * 2 * n);
  a.n = n; a.n1 = n1; a.max_sweeps = max_sweeps; a.max_assets = max_assets < 0 ? -1 : max_assets; a.spl = sweeps_per_launch;
  HIP_OK(hipMemsetAsync(state, 0, encd_state_bytes(P, n), st));
  HIP_OK(hipMemsetAsync(theta, 0, (size_t)P * n1 * n * sizeof(double), st));
  HIP_OK(hipMemsetAsync(sweeps, 0, (size_t)P * n1 * sizeof(int), st));
  HIP_OK(hipMemsetAsync(nnz, 0, (size_t)P * n1 * sizeof(int), st));
  // every launch runs at least one sweep of every path that is not done
  const long long most = ((long long)n1 * max_sweeps + sweeps_per_launch - 1) / sweeps_per_launch + 1;
  std::vector<int> flags((size_t)4 * P);
  struct Events {                                  // (destroyed on a throw as well)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  } ev;
  if (ms) { HIP_OK(hipEventCreate(&ev.e0)); HIP_OK(hipEventCreate(&ev.e1)); }
  int launches = 0;
  for (bool all = false; !all;) {
    if (launches >= most)
      dlap_throw_hip(hipErrorUnknown, "en_paths: paths not done after every sweep they can run", __FILE__, __LINE__);
    if (ms) HIP_OK(hipEventRecord(ev.e0, st));
    launch(a, P, st);
    if (ms) HIP_OK(hipEventRecord(ev.e1, st));
    ++launches;
    HIP_OK(hipMemcpyAsync(flags.data(), a.st_i, flags.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (ms) {
      float t = 0.f;
      HIP_OK(hipEventElapsedTime(&t, ev.e0, ev.e1));
      ms->push_back(t);
    }
    all = true;
    for (long long p = 0; p < P && all; ++p) all = flags[(size_t)4 * p + 2] != 0;
  }
  if (updates) {
    updates->resize((size_t)P);
    for (long long p = 0; p < P; ++p) (*updates)[(size_t)p] = flags[(size_t)4 * p + 3];
  }
  return launches;
}
