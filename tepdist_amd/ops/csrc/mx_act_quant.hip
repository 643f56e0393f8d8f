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

template <bool ROUNDTRIP>
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
  const unsigned byte = mxq_scale_byte(amax);

  unsigned q[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned two = mxq_e4m3(v[j] & 0xffffu, byte) |
                         (mxq_e4m3(v[j] >> 16, byte) << 8);
    if (j & 1) q[j >> 1] |= two << 16;
    else q[j >> 1] = two;
  }

  if constexpr (ROUNDTRIP) {
    *reinterpret_cast<bf16x8*>(out + row * ldo + 8 * c) =
        dq_fp8(q[0], q[1], mx_scale(byte));
  } else {
    *reinterpret_cast<uint2*>(codes + row * ldc + 8 * c) =
        make_uint2(q[0], q[1]);
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
                  hipStream_t stream) {
  auto a = [](const void* p, int n) {
    return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0;
  };
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
  if (!roundtrip && (!a(codes, 8) || ldc < K || (ldc & 7) || lds < K / 32))
    throw std::runtime_error(
        "mx_act_quant: codes need an 8-byte-aligned base and rows, scale "
        "rows K / 32 bytes");
  const int K8 = K / 8;
  const int64_t total = (int64_t)M * K8;
  const int64_t blocks = (total + MXQ_THREADS - 1) / MXQ_THREADS;
  if (blocks > INT32_MAX)
    throw std::runtime_error("mx_act_quant: M * K is too large for one grid");
  const int dword = !roundtrip && K % 128 == 0 && a(scales, 4) &&
                    (lds & 3) == 0;
#define MXQ_GO(RT)                                                          \
  hipLaunchKernelGGL((mx_act_quant_kernel<RT>), dim3((unsigned)blocks),     \
                     dim3(MXQ_THREADS), 0, stream,                          \
                     static_cast<const bf16_t*>(x),                         \
                     static_cast<uint8_t*>(codes),                          \
                     static_cast<uint8_t*>(scales),                         \
                     static_cast<bf16_t*>(out), total, K8, ldx, ldc, lds,   \
                     ldo, dword)
  if (roundtrip) MXQ_GO(true); else MXQ_GO(false);
#undef MXQ_GO
}

}  // namespace tepdist
