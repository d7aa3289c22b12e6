// Device helpers shared by the quantile-sort kernels (k_qsort.hip, k_qsort2.hip, k_qtree.hip,
// k_qtree_weight.hip): the
// order-preserving float -> uint32 key map, the key load from the compacted panel and
// (k_qtree.hip) the wave's step of the radix select.
#pragma once
#include "common.h"
#include "panel_view.h"

DLAP_DEV uint32_t qkey_u32(float x) {
  uint32_t b = __float_as_uint(x);
  b = b == 0x80000000u ? 0u : b;                       // -0.0 -> +0.0
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
// the key's value; k16: a 16-bit (bf16) key in the high half
DLAP_DEV float qkey_f32(uint32_t u, bool k16) {
  if (k16) return __uint_as_float((u ^ ((u >> 31) ? 0x80000000u : 0xFFFF0000u)) & 0xFFFF0000u);
  return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// key of compact row r: panel column col of a characteristic block, else the dense array ext [N]
template <bool F32>
DLAP_DEV uint32_t qkey_load(const PanelView& a, bool is_char, int col, const float* ext, int r) {
  if (is_char) {
    if constexpr (F32) return qkey_u32(gp(reinterpret_cast<const float*>(a.X))[(size_t)r * a.KP + col]);
    else {
      uint32_t h = gp(reinterpret_cast<const u16*>(a.X))[(size_t)r * a.KP + col];
      h = h == 0x8000u ? 0u : h;
      return (h ^ ((h >> 15) ? 0xFFFFu : 0x8000u)) << 16;
    }
  }
  const int i = gp(a.rowti)[r].y;
  return qkey_u32(gp(ext)[i]);
}

// Full-width key of compact row r = (t, i) in key column c of a call (c < F: panel column c, else the
// dense array c - F of extra [E][T][N]): qkey_u32 of the fp32 value, a bf16 characteristic widened
// exactly first. Against qkey_u32 of a breakpoint this is the float comparison for any breakpoint
// value. Its high half is qkey_load's bf16 key; the low half is 0xFFFF for a negative value where
// qkey_load leaves 0, which is what the comparison with a full-width negative breakpoint needs
// (k_qtree_weight.hip; the sort kernels compare 16-bit prefixes and keep qkey_load).
template <bool F32>
DLAP_DEV uint32_t qkey_row(const PanelView& a, int c, const float* extra, int t, int r, int i) {
  float x;
  if (c < a.F) {
    if constexpr (F32) x = gp(reinterpret_cast<const float*>(a.X))[(size_t)r * a.KP + c];
    else x = __uint_as_float((uint32_t)gp(reinterpret_cast<const u16*>(a.X))[(size_t)r * a.KP + c] << 16);
  } else {
    x = gp(extra)[((size_t)(c - a.F) * a.T + t) * a.N + i];
  }
  return qkey_u32(x);
}

// One wave's step of the multi-level radix select (k_qsort2.hip's scan): the histogram h of
// nbins <= 256 bins holds the rows of a breakpoint's group by their digit at this level, rk is the
// breakpoint's residual rank within the group (rk < the group's rows). Exactly one lane finds the
// bin that holds rank rk and returns true with dg = the bin, below = the rows in the bins below it
// and in_bin = the rows in it. Lane l reads the bins 4 l .. 4 l + 3.
DLAP_DEV bool qsel_wave_scan(const uint32_t* h, int nbins, uint32_t rk, int lane, uint32_t& dg, uint32_t& below,
                             uint32_t& in_bin) {
  const int b0 = 4 * lane;
  const uint32_t c0 = b0 < nbins ? h[b0] : 0u, c1 = b0 + 1 < nbins ? h[b0 + 1] : 0u;
  const uint32_t c2 = b0 + 2 < nbins ? h[b0 + 2] : 0u, c3 = b0 + 3 < nbins ? h[b0 + 3] : 0u;
  const uint32_t sb = c0 + c1 + c2 + c3;
  uint32_t inc = sb;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  uint32_t cb = inc - sb;                              // rows in the bins below this lane's
  if (!(cb <= rk && rk < inc)) return false;
  dg = (uint32_t)b0; in_bin = c0;
  if (rk >= cb + c0) { cb += c0; ++dg; in_bin = c1;
    if (rk >= cb + c1) { cb += c1; ++dg; in_bin = c2;
      if (rk >= cb + c2) { cb += c2; ++dg; in_bin = c3; } } }
  below = cb;
  return true;
}
