// The dropout keep-word generator's body, shared by k_dropmask (k_mlp.hip) and the mask blocks of
// the fused backward tail (k_lstm_tail, k_rnn.hip): both write the same words to the same addresses.
#pragma once
#include "mlp.h"

// Keep words of lane `lane` of up to U tiles tile0, tile0 + stride, ... (those below tile_end) for
// dropout step `step`, every SDF layer, into that step's parity half of J.gbits (split layout,
// keep_word). Every row-index load is issued before the first hash: a caller with few waves per
// SIMD (the tail) pays one memory round trip per U tiles. The caller checks J.dropout > 0.
template <int U>
DLAP_DEV void dropmask_tiles(const MlpJob& J, int nl_sdf, uint32_t step, int tile0, int stride, int tile_end,
                             int lane) {
  const int q = lane >> 4;
  const uint32_t thr16 = (uint32_t)(J.dropout * 65536.f + 0.5f);
  int2 ti[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int tile = min(tile0 + u * stride, tile_end - 1);
#pragma unroll
    for (int b = 0; b < 2; ++b) ti[u][b] = gp(J.rowti)[min(tile * 32 + 16 * b + (lane & 15), J.R - 1)];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int tile = tile0 + u * stride;
    if (tile >= tile_end) break;
    uint32_t rowmix[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int r = tile * 32 + 16 * b + (lane & 15);
      // rows beyond R hash as dense row -1, as the towers do (their words are never used)
      rowmix[b] = row_mix(r < J.R ? (uint32_t)(ti[u][b].x * J.N + ti[u][b].y) : 0xFFFFFFFFu);
    }
    const auto dst = gp(const_cast<uint32_t*>(J.gbits)) + (size_t)(step & 1u) * J.gb_half + (size_t)tile * nl_sdf * 64 + lane;
    for (int j = 0; j < nl_sdf; ++j) dst[64 * j] = keep_word<4>(dropout_key(J.seed, step, j), rowmix, thr16, q);
  }
}
