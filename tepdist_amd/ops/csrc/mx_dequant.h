// Register dequantizers of OCP MX codes shared by skinny_mx_gemm.hip and
// mx_gemm.hip: eight codes and the block's fp32 scale to one bf16x8 MFMA
// fragment, with v_cvt_scalef32_pk_bf16_fp4 / _fp8.
#pragma once

#include "common.h"

namespace tepdist {
namespace {

DEV_INLINE unsigned mx_u(bf16x2 v) { return __builtin_bit_cast(unsigned, v); }

// eight e2m1 codes (low nibble first) times s -> bf16x8
DEV_INLINE bf16x8 dq_fp4(unsigned c, float s) {
  u32x4 r;
  r[0] = mx_u(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, 0));
  r[1] = mx_u(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, 1));
  r[2] = mx_u(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, 2));
  r[3] = mx_u(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, 3));
  return __builtin_bit_cast(bf16x8, r);
}

// eight e4m3 codes (low byte first) times s -> bf16x8
DEV_INLINE bf16x8 dq_fp8(unsigned c0, unsigned c1, float s) {
  u32x4 r;
  r[0] = mx_u(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c0, s, false));
  r[1] = mx_u(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c0, s, true));
  r[2] = mx_u(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c1, s, false));
  r[3] = mx_u(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c1, s, true));
  return __builtin_bit_cast(bf16x8, r);
}

// e8m0 byte -> fp32 scale (bytes 0 and 255 never occur, ops/mx.py)
DEV_INLINE float mx_scale(unsigned byte) {
  return __builtin_bit_cast(float, byte << 23);
}

}  // namespace
}  // namespace tepdist
