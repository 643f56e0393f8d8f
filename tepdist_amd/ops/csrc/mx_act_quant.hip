// MXFP8 activation quantizer for gfx950: x[M, K] bf16 (rows strided, K % 32
// == 0) to e4m3 codes [M, K] and one e8m0 scale byte per 32 k, by exactly the
// rule of ops/mx.py's mx_quantize(x, "mxfp8"):
//   scale byte = clamp(biased exponent of the block amax - 8, 10, 246), 127
//   for an all-zero block; elements over 2^(byte - 127), clamped to +-448 and
//   rounded to nearest even into e4m3, subnormal codes included; the NaN
//   codes are never emitted.
// The element rule is mxq_e4m3 of mx_gemm_a8_plan.h, integer arithmetic on the
// bf16 pattern: the same lines run on the host, where all 65 280 finite
// patterns are compared with the Python quantizer, and nothing depends on the
// denormal mode or on how a hardware convert saturates. ROUNDTRIP writes
// instead the dequantized bf16 values (dq_fp8 of mx_dequant.h: an e4m3
// element times an in-range scale is exact in bf16).
//
// Work split. One thread per 8 consecutive k: one 16-byte load. The four
// adjacent lanes of a quad own one MX block; K / 8 is a multiple of 4, so a
// quad never straddles a row and is wholly inside or outside the M * K / 8
// threads of the problem. The block amax is the integer maximum of the 15
// magnitude bits over the quad, two quad_perm DPP steps (xor 1, xor 2). Each
// lane stores its 8 code bytes in one 8-byte store. Scale bytes: where K %
// 128 == 0 the 16 lanes of a DPP row are four consecutive blocks 4j .. 4j + 3
// of one row, their bytes are gathered into the row's lane 0 by two shuffles
// and stored as one dword if the scale rows are 4-byte aligned; otherwise
// lane 0 of each quad stores its byte. Rows >= M are never touched (no thread
// exists for them). No LDS, no atomics, one launch.
//
// MXFP4 (XBITS = 4): mx_quantize(x, "mxfp4") by mxq_scale_byte4 / mxq_e2m1 of
// the same header (scale byte = clamp(biased exponent of the amax - 2, 2,
// 252), elements saturated at +-6, ties to the even code), codes [M, K / 2]
// with even k in the low nibble. Same split, load, amax and scale stores; a
// lane's 8 codes are one dword, and the quad's 16 bytes leave as two 8-byte
// stores: each even lane takes its odd neighbour's dword by one quad_perm DPP
// and stores the pair. The alternative, one 16-byte store by the quad's lane
// 0, needs three DPP moves and 16-byte-aligned code rows; the pair store
// keeps the 8-byte rule of the mxfp8 codes (the same out= views are taken)
// and a wave still writes 256 contiguous bytes. The round trip is dq_fp4 of
// mx_dequant.h: an e2m1 element times an in-range scale is exact in bf16.

#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "mx_dequant.h"
#include "mx_gemm_a8_plan.h"

namespace tepdist {

namespace {

constexpr int MXQ_THREADS = 256;

template <int CTRL>
DEV_INLINE unsigned mxq_quad(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf,
                                               true);
}

template <bool ROUNDTRIP, int XBITS>
__launch_bounds__(MXQ_THREADS) __global__
void mx_act_quant_kernel(const bf16_t* __restrict__ x,
                         uint8_t* __restrict__ codes,
                         uint8_t* __restrict__ scales,
                         bf16_t* __restrict__ out, int64_t total, int K8,
                         int64_t ldx, int64_t ldc, int64_t lds, int64_t ldo,
                         int dword_scales) {
  const int64_t idx = (int64_t)blockIdx.x * MXQ_THREADS + threadIdx.x;
  if (idx >= total) return;  // whole quads (and, K % 128 == 0, DPP rows)
  const int64_t row = idx / K8;
  const int c = (int)(idx - row * K8);  // this lane's 8 k: 8 c .. 8 c + 7
  const u32x4 v = *reinterpret_cast<const u32x4*>(x + row * ldx + 8 * c);

  unsigned amax = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned lo = v[j] & 0x7fffu, hi = (v[j] >> 16) & 0x7fffu;
    amax = max(amax, max(lo, hi));
  }
  amax = max(amax, mxq_quad<0xB1>(amax));  // quad_perm [1, 0, 3, 2]
  amax = max(amax, mxq_quad<0x4E>(amax));  // quad_perm [2, 3, 0, 1]
  const unsigned byte =
      XBITS == 4 ? mxq_scale_byte4(amax) : mxq_scale_byte(amax);

  unsigned q[2] = {0, 0};  // XBITS == 4: q[0] alone, eight nibbles
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (XBITS == 4) {
      q[0] |= (mxq_e2m1(v[j] & 0xffffu, byte) |
               (mxq_e2m1(v[j] >> 16, byte) << 4)) << (8 * j);
    } else {
      const unsigned two = mxq_e4m3(v[j] & 0xffffu, byte) |
                           (mxq_e4m3(v[j] >> 16, byte) << 8);
      q[j >> 1] |= two << (16 * (j & 1));
    }
  }

  if constexpr (ROUNDTRIP) {
    *reinterpret_cast<bf16x8*>(out + row * ldo + 8 * c) =
        XBITS == 4 ? dq_fp4(q[0], mx_scale(byte))
                   : dq_fp8(q[0], q[1], mx_scale(byte));
  } else {
    if constexpr (XBITS == 4) {
      const unsigned odd = mxq_quad<0xF5>(q[0]);  // quad_perm [1, 1, 3, 3]
      if ((threadIdx.x & 1) == 0)
        *reinterpret_cast<uint2*>(codes + row * ldc + 4 * c) =
            make_uint2(q[0], odd);
    } else {
      *reinterpret_cast<uint2*>(codes + row * ldc + 8 * c) =
          make_uint2(q[0], q[1]);
    }
    uint8_t* sp = scales + row * lds + (c >> 2);
    if (dword_scales) {
      unsigned g = byte | ((unsigned)__shfl_down((int)byte, 4, 64) << 8);
      g |= (unsigned)__shfl_down((int)g, 8, 64) << 16;
      if ((threadIdx.x & 15) == 0) *reinterpret_cast<unsigned*>(sp) = g;
    } else if ((threadIdx.x & 3) == 0) {
      *sp = (uint8_t)byte;
    }
  }
}

}  // namespace

void mx_act_quant(const void* x, void* codes, void* scales, void* out, int M,
                  int K, int64_t ldx, int64_t ldc, int64_t lds, int64_t ldo,
                  hipStream_t stream, int x_bits) {
  auto a = [](const void* p, int n) {
    return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0;
  };
  if (x_bits != 8 && x_bits != 4)
    throw std::runtime_error("mx_act_quant: x_bits must be 8 or 4");
  if (M < 1 || K < 32 || K % 32)
    throw std::runtime_error(
        "mx_act_quant: M must be positive and K a positive multiple of 32");
  if (!x || !a(x, 16) || ldx < K || (ldx & 7))
    throw std::runtime_error(
        "mx_act_quant: x needs a 16-byte-aligned base and rows");
  const bool roundtrip = out != nullptr;
  if (roundtrip == (codes != nullptr) || (codes != nullptr) !=
      (scales != nullptr))
    throw std::runtime_error(
        "mx_act_quant: give either codes and scales or the round-trip out");
  if (roundtrip && (!a(out, 16) || ldo < K || (ldo & 7)))
    throw std::runtime_error(
        "mx_act_quant: out needs a 16-byte-aligned base and rows");
  if (!roundtrip && (!a(codes, 8) || ldc < K * x_bits / 8 || (ldc & 7) ||
                     lds < K / 32))
    throw std::runtime_error(
        "mx_act_quant: codes need an 8-byte-aligned base and rows (a byte "
        "stride that is a multiple of 8, at least K * bits / 8), scale rows "
        "K / 32 bytes");
  const int K8 = K / 8;
  const int64_t total = (int64_t)M * K8;
  const int64_t blocks = (total + MXQ_THREADS - 1) / MXQ_THREADS;
  if (blocks > INT32_MAX)
    throw std::runtime_error("mx_act_quant: M * K is too large for one grid");
  const int dword = !roundtrip && K % 128 == 0 && a(scales, 4) &&
                    (lds & 3) == 0;
#define MXQ_GO(RT, XX)                                                      \
  hipLaunchKernelGGL((mx_act_quant_kernel<RT, XX>), dim3((unsigned)blocks), \
                     dim3(MXQ_THREADS), 0, stream,                          \
                     static_cast<const bf16_t*>(x),                         \
                     static_cast<uint8_t*>(codes),                          \
                     static_cast<uint8_t*>(scales),                         \
                     static_cast<bf16_t*>(out), total, K8, ldx, ldc, lds,   \
                     ldo, dword)
  if (x_bits == 4) {
    if (roundtrip) MXQ_GO(true, 4); else MXQ_GO(false, 4);
  } else {
    if (roundtrip) MXQ_GO(true, 8); else MXQ_GO(false, 8);
  }
#undef MXQ_GO
}

}  // namespace tepdist
