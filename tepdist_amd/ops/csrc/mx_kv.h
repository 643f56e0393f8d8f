// Register pieces of the MXFP8 KV cache (ops/mx.py MXCache) shared by
// decode_attention_mx.hip and prefill_attention.hip: the quantizer of a new
// row, 8 elements per lane with the 32-element block spread over a quad, and
// the fp32 dequantizer of 8 codes.
#pragma once

#include "common.h"
#include "mx_dequant.h"
#include "mx_gemm_a8_plan.h"

namespace tepdist {
namespace {

template <int CTRL>
DEV_INLINE unsigned mxkv_quad(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf,
                                               true);
}

// mx.mx_quantize(row, "mxfp8") of a lane's 8 bf16 elements (four packed
// words, low half first): the codes in c0 (elements 0..3) and c1, the
// block's scale byte in `byte`. The four lanes of a quad hold one block and
// must all be active; the amax is the integer maximum of the magnitude bits,
// the element rule mxq_e4m3 (no hardware saturating convert).
DEV_INLINE void mxkv_quant8(unsigned w0, unsigned w1, unsigned w2,
                            unsigned w3, unsigned& c0, unsigned& c1,
                            unsigned& byte) {
  const unsigned w[4] = {w0, w1, w2, w3};
  unsigned amax = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    amax = max(amax, max(w[j] & 0x7fffu, (w[j] >> 16) & 0x7fffu));
  amax = max(amax, mxkv_quad<0xB1>(amax));  // quad_perm [1, 0, 3, 2]
  amax = max(amax, mxkv_quad<0x4E>(amax));  // quad_perm [2, 3, 0, 1]
  byte = mxq_scale_byte(amax);
  unsigned two[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    two[j] = mxq_e4m3(w[j] & 0xffffu, byte) |
             (mxq_e4m3(w[j] >> 16, byte) << 8);
  c0 = two[0] | (two[1] << 16);
  c1 = two[2] | (two[3] << 16);
}

// eight e4m3 codes (low byte first) times 2^(byte - 127) -> fp32, exact:
// v_cvt_scalef32_pk_f32_fp8 converts two codes and applies the scale
DEV_INLINE void mxkv_dq8(unsigned c0, unsigned c1, unsigned byte, float* f) {
  const float s = mx_scale(byte);
  const auto a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c0, s, false);
  const auto b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c0, s, true);
  const auto c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c1, s, false);
  const auto d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c1, s, true);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
  f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
}

}  // namespace
}  // namespace tepdist
