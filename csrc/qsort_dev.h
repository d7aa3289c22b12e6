// Device helpers shared by the quantile-sort kernels (k_qsort.hip, k_qsort2.hip): the
// order-preserving float -> uint32 key map and the key load from the compacted panel.
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
