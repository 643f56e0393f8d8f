// Host-side plan of one linear on MX weights and MX activations:
// y[M, N] = dq(Xq)[M, K] . dq(W)[N, K]^T for any M >= 1. W is OCP MX codes
// (e2m1 or e4m3), Xq e4m3 codes [M, K] or, against e2m1 weights only, e2m1
// codes [M, K / 2]; both carry one e8m0 scale byte per 32 k of a row
// (ops/mx.py). Plain C++17, no HIP include, like the other plans,
// whose epilogue enum and tile rule it shares: mx_gemm_a8.hip launches what
// this returns and the extension binds it as `mx_gemm_a8_plan`. It also holds
// the activation quantizer's element rule (mx_act_quant.hip), written in
// integers so that the host and the device run the same lines.
#pragma once

#include <cstdint>

#include "mx_gemm_plan.h"

#if defined(__HIP__)  // a HIP translation unit: callable from kernels too
#define MXA8_HD __attribute__((host)) __attribute__((device)) inline
#else
#define MXA8_HD inline
#endif

namespace tepdist {

// w_bits: 4 (e2m1) or 8 (e4m3) weights; x_bits: 8 (e4m3) or 4 (e2m1)
// activations, the latter with e2m1 weights only (W8A4 is not built). ld_*:
// row strides in bytes of the weight's and the activation's code and scale
// arrays. Tile rule, stages and
// the K-tile are those of mx_gemm_plan (mx_tiled): 128 where its grid has at
// least 256 blocks. Bases and the rows of the residual and y are checked by
// the launcher, which alone sees them.
inline MxGemmPlan mx_gemm_a8_plan(int M, int N, int K, int w_bits,
                                  int64_t ld_wcodes, int64_t ld_wscales,
                                  int64_t ld_xcodes, int64_t ld_xscales,
                                  int epi, int tile_override,
                                  int x_bits = 8) {
  auto refuse = [](const char* why) { return MxGemmPlan{0, 0, 0, why}; };
  const MxGemmPlan p = mx_gemm_plan(M, N, K, w_bits, ld_wcodes, ld_wscales,
                                    epi, tile_override);
  if (p.why_not) return p;
  if (x_bits != 8 && x_bits != 4)
    return refuse("x_bits must be 8 (mxfp8) or 4 (mxfp4)");
  if (x_bits == 4 && w_bits != 4)
    return refuse("mxfp4 activations need mxfp4 weights (W8A4 is not built)");
  if (x_bits == 4 && (ld_xcodes < K / 2 || (ld_xcodes & 15)))
    return refuse("mxfp4 activation code rows must be 16-byte aligned (a byte "
                  "stride that is a multiple of 16, at least K / 2)");
  if (x_bits == 8 && (ld_xcodes < K || (ld_xcodes & 15)))
    return refuse("activation code rows must be 16-byte aligned (a byte "
                  "stride that is a multiple of 16, at least K)");
  if (ld_xscales < K / 32 || (ld_xscales & 3))
    return refuse("activation scale rows must be 4-byte aligned (a byte "
                  "stride that is a multiple of 4, at least K / 32)");
  return p;
}

// -- the MXFP8 activation quantizer's rule (ops/mx.py mx_quantize, "mxfp8") --
// on bf16 bit patterns. A finite bf16 is sig * 2^(E - 134) with E = max(e, 1)
// and sig = m + 128 (e != 0) or m (subnormal), e / m its exponent and
// mantissa fields.

// scale byte of a block from the largest |bits| of its elements
MXA8_HD unsigned mxq_scale_byte(unsigned amax_bits) {
  if (amax_bits == 0) return 127;
  const int b = (int)(amax_bits >> 7) - 8;  // a subnormal amax clamps anyway
  return b < 10 ? 10 : b > 246 ? 246 : b;
}

// e4m3 code of one element under its block's scale byte: the element over
// 2^(byte - 127) is sig * 2^(s - 7) with s = E - byte <= 8 (byte >= E_amax -
// 8), clamped to 448 and rounded to nearest even. A normal result has the
// code exponent s + 7 and the top three mantissa bits, rounded with the carry
// running into the exponent; 0x7e (448) caps what 448 < v < 512 would round
// to. Below 2^-6 the code counts units of 2^-9: sig >> -(s + 2), rounded.
MXA8_HD unsigned mxq_e4m3(unsigned bits, unsigned byte) {
  const unsigned sign = (bits >> 8) & 0x80, e = (bits >> 7) & 0xff,
                 m = bits & 0x7f;
  const int s = (int)(e ? e : 1) - (int)byte;
  unsigned code;
  if (e != 0 && s >= -6) {
    const unsigned t = ((unsigned)(s + 7) << 7) | m;
    code = (t + 7 + ((t >> 4) & 1)) >> 4;
    if (code > 0x7e) code = 0x7e;
  } else {
    const unsigned sig = e ? m + 128 : m;
    const int sh = -(s + 2);                 // >= 5
    if (sh > 9) {
      code = 0;                              // sig / 2^sh < 1/2
    } else {
      const unsigned half = 1u << (sh - 1), rem = sig & (2 * half - 1);
      code = sig >> sh;
      code += (rem > half) || (rem == half && (code & 1));
    }
  }
  return sign | code;
}

// -- the MXFP4 rule (mx_quantize, "mxfp4"): the block's elements over
// 2^(byte - 127) lie below 8, saturate at 6 and round to the nearest e2m1
// value, ties to the even code --

// scale byte: biased exponent of the amax - 2, in [2, 252]
MXA8_HD unsigned mxq_scale_byte4(unsigned amax_bits) {
  if (amax_bits == 0) return 127;
  const int b = (int)(amax_bits >> 7) - 2;  // a subnormal amax clamps anyway
  return b < 2 ? 2 : b > 252 ? 252 : b;
}

// e2m1 code (4 bits) of one element: the scaled element is sig * 2^(s - 7)
// with s = E - byte <= 2. From 1.0 up it is a normal code with exponent
// field s + 1 and the top mantissa bit, rounded with the carry running into
// the exponent; 7 (6.0) caps what lies above. Below 1.0 the code counts
// halves: sig >> (6 - s), rounded, which reaches code 2 (1.0) at most. Zero
// keeps code 0 whatever its sign; a nonzero element that rounds to zero keeps
// its sign, as the Python quantizer has it.
//
// That rule takes both of its paths inside most waves (a third of a block's
// elements lie below 1.0), so from byte 9 up, which is every block whose amax
// is at least 2^-116, a branch-free form of it runs instead: the magnitude
// bits minus (byte - 127) << 7 are the bf16 pattern of the scaled element
// (negative, or an exponent field <= 118 for a subnormal input: far below
// 0.25 either way), patterns order as values do, and the code is the number
// of the seven midpoints 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 it has passed,
// a tie passing only onto an even code.
MXA8_HD unsigned mxq_e2m1(unsigned bits, unsigned byte) {
  const unsigned e = (bits >> 7) & 0xff, m = bits & 0x7f;
  const unsigned sign = (bits & 0x7fff) ? (bits >> 12) & 8 : 0;
  if (byte >= 9) {
    const int t = (int)(bits & 0x7fff) - ((int)byte - 127) * 128;
    return sign | (unsigned)((t > 0x3e80) + (t >= 0x3f40) + (t > 0x3fa0) +
                             (t >= 0x3fe0) + (t > 0x4020) + (t >= 0x4060) +
                             (t > 0x40a0));
  }
  const int s = (int)(e ? e : 1) - (int)byte;
  unsigned code;
  if (e != 0 && s >= 0) {
    const unsigned t = ((unsigned)(s + 1) << 7) | m;
    code = (t + 31 + ((t >> 6) & 1)) >> 6;
    if (code > 7) code = 7;
  } else {
    const unsigned sig = e ? m + 128 : m;
    const int sh = 6 - s;                    // >= 7
    if (sh > 9) {
      code = 0;                              // sig / 2^sh < 1/2
    } else {
      const unsigned half = 1u << (sh - 1), rem = sig & (2 * half - 1);
      code = sig >> sh;
      code += (rem > half) || (rem == half && (code & 1));
    }
  }
  return sign | code;
}

}  // namespace tepdist
