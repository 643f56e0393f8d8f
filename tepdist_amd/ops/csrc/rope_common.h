// The one place RoPE angles are computed on the device (rotate-half
// convention: element d in [0, D/2) pairs with d + D/2; freq_d =
// theta^(-2d/D), angle = pos * freq_d). rope_kernel (prefill, llama_ops.hip)
// and the decode kernel (decode_attention.hip) both call it, so a row
// rotated at prefill and one rotated at decode use the same arithmetic.
#pragma once

#include "common.h"

// neg2_over_d = -2/D, ltheta = logf(theta), both computed on the host.
DEV_INLINE void rope_sincos(int pos, int d, float neg2_over_d, float ltheta,
                            float* sn, float* cs) {
  const float freq = __expf(ltheta * neg2_over_d * d);
  __sincosf(pos * freq, sn, cs);
}
