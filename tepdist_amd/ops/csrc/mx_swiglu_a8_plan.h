// Host-side plan of the fused SwiGLU gate/up GEMM on MX weights and MX
// activations: h[M, I] = silu(dq(Xq) . dq(Wg)^T) * (dq(Xq) . dq(Wu)^T), h
// written as bf16 or as MX codes and scale bytes. Plain C++17, no HIP
// include, like the other plans: mx_swiglu_a8.hip launches what this returns
// and the extension binds it as `mx_swiglu_a8_plan`. The operand rules for
// Xq and for both weights are mx_gemm_a8_plan's, which is called and not
// changed.
#pragma once

#include <cstdint>

#include "mx_gemm_a8_plan.h"

namespace tepdist {

// Gate and up are MXWeights [I, K] / [up_I, up_K] of w_bits / up_bits with
// code and scale row strides ld_w* / ld_u* in bytes; they must agree in all
// of it, so that one pair of strides serves the paired weight tile. out_bits:
// 0 = bf16 h, 8 = e4m3, 4 = e2m1 codes (row stride ld_ocodes bytes) with one
// scale byte per 32 hidden columns (ld_oscales). The returned `tile` names
// the token rows of a block: 128 tokens x 64 hidden columns, or 64 x 32.
// Either way a block stages `tile` weight rows (gate rows, then the up rows
// of the same columns), so the choice is mx_gemm_plan's fill rule on the 2 I
// weight rows, and blocks = ceil(M / tile) * ceil(I / (tile / 2)).
inline MxGemmPlan mx_swiglu_a8_plan(int M, int I, int K, int w_bits,
                                    int64_t ld_wcodes, int64_t ld_wscales,
                                    int up_I, int up_K, int up_bits,
                                    int64_t ld_ucodes, int64_t ld_uscales,
                                    int64_t ld_xcodes, int64_t ld_xscales,
                                    int epi, int tile_override, int x_bits,
                                    int out_bits, int64_t ld_ocodes,
                                    int64_t ld_oscales) {
  auto refuse = [](const char* why) { return MxGemmPlan{0, 0, 0, why}; };
  if (epi != SK_NONE)
    return refuse("swiglu takes no bias, no residual and no gelu");
  if (up_I != I || up_K != K || up_bits != w_bits)
    return refuse("gate and up must have one format and one shape");
  if (ld_ucodes != ld_wcodes || ld_uscales != ld_wscales)
    return refuse("gate and up must have the same code and scale row strides");
  if (I < 1 || I > INT32_MAX / 2) return refuse("I must be in 1 .. 2^30 - 1");
  const MxGemmPlan p =
      mx_gemm_a8_plan(M, 2 * I, K, w_bits, ld_wcodes, ld_wscales, ld_xcodes,
                      ld_xscales, epi, tile_override, x_bits);
  if (p.why_not) return p;
  if (out_bits != 0 && out_bits != 8 && out_bits != 4)
    return refuse("out_bits must be 0 (bf16), 8 (mxfp8) or 4 (mxfp4)");
  if (out_bits != 0) {
    if (I % 32)
      return refuse("a quantized output needs I to be a multiple of 32");
    if (ld_ocodes < (int64_t)I * out_bits / 8 || (ld_ocodes & 7))
      return refuse("output code rows must be 8-byte aligned (a byte stride "
                    "that is a multiple of 8, at least I * out_bits / 8)");
    if (ld_oscales < I / 32)
      return refuse("output scale rows must hold I / 32 bytes");
  }
  const int bh = p.tile / 2;
  const int64_t blocks =
      ((int64_t)M + p.tile - 1) / p.tile * (((int64_t)I + bh - 1) / bh);
  return MxGemmPlan{p.tile, p.stages, (int)blocks, nullptr};
}

}  // namespace tepdist
