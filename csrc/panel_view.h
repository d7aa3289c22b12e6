// The resident panel of one split as the panel-only kernels see it (k_qsort.hip, k_qsort2.hip,
// k_linport.hip, k_xgram.hip; k_knock.hip's reduction reads its panel side through it): the
// compacted rows the engine keeps on the device, no model, job table or graph. Their argument structs embed it as the first member `pv`; the engine fills it in
// one place (Engine::panel_view). A pass reads the fields it needs (k_xgram reads no rowti or N).
#pragma once
#include "common.h"

struct PanelView {
  const void* X;          // [R][KP] bf16 bits, or fp32 when fp32 != 0; columns [0, F) are the characteristics,
                          // columns >= F are not read as data
  int KP, fp32, F;
  const float* Rc;        // [R] returns of the compact rows
  const int2* rowti;      // [R] (t, i)
  const int* row_ptr;     // [T+1] first compact row of each period
  int T, N;
};
