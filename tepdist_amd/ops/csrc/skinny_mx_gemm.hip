// Skinny-M weight-streaming GEMM on OCP MX weights for gfx950:
//   y[M, N] = epi(x[M, K] . dq(W)[N, K]^T),  1 <= M <= 64, x / bias /
//   residual / y bf16, fp32 accumulate, one rounding,
// the dual form y = silu(x . dq(Wg)^T) * (x . dq(Wu)^T), and a stand-alone
// dequantizer. W is e2m1 (mxfp4) or e4m3 (mxfp8) codes with one e8m0 scale
// byte per 32 consecutive k of a row, in the interchange layout of
// ops/mx.py; nothing is repacked.
//
// An element times a power of two is exact in bf16 (mx.py clamps the scale
// so that it is also normal), so the kernel computes exactly what
// skinny_gemm.hip computes on the dequantized weights; it only reads 3.8x or
// 1.9x fewer bytes to get there. The skeleton is that kernel's: weights are
// the A operand of mfma_f32_16x16x32_bf16 and never touch LDS, MT = 1, 2 or
// 4 token fragments reuse every weight fragment, K is split over the waves
// of a block, loads run in two ping-pong register sets with a clamped
// unconditional look-ahead, partial tiles are summed through LDS in wave
// order (bit-reproducible, no atomics, no workspace). What differs:
//
// * A K-step is 128 for both formats, four MFMAs. Lane 16g + i owns row i
//   of a tile and elements 32g .. 32g + 31 of the step: exactly one MX
//   block, so a lane needs one scale per step and tile. The block is one
//   16-byte load (e2m1) or two (e4m3); the four lanes of a row fetch 64 or
//   128 contiguous bytes. The scale is a byte load at scales[row][4 step +
//   g]: one instruction, and `byte << 23` is the fp32 scale (bytes 0 and 255
//   never occur). The step's scale dword with a per-lane byte extract costs
//   the same four bytes of traffic per row and one VALU op more.
// * Dequantization happens in registers, once per weight fragment:
//   v_cvt_scalef32_pk_bf16_fp4 / _fp8 turn two codes and the scale into a
//   bf16 pair, four of them make the bf16x8 A fragment of one MFMA, 16 the
//   four fragments of a step. Dword d of an e2m1 block (dwords 2d, 2d + 1
//   of an e4m3 block) feeds MFMA d, i.e. k = 32g + 8d .. 32g + 8d + 7; the
//   fragment is then reused over all MT token fragments.
// * x is read in the same k order: 64 contiguous bytes per lane and step,
//   16-byte load d feeding MFMA d. As in the bf16 kernel the permutation of
//   k inside a step is free because both operands share it.
//
// The reduction and the epilogue are the bf16 kernel's, repeated here so
// that skinny_gemm.hip stays byte for byte what its measurements describe.
// The native v_mfma_scale_f32_16x16x128_f8f6f4 path (quantized activations,
// other numerics) is not built.

#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "mx_dequant.h"
#include "skinny_mx_plan.h"

namespace tepdist {

namespace {

constexpr int MX_MAX_THREADS = skinny::MAX_WAVES * WAVE;

DEV_INLINE float mx_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

template <int BITS, int MT, int RT, bool DUAL>
__launch_bounds__(MX_MAX_THREADS) __global__
void skinny_mx_kernel(const bf16_t* __restrict__ x,
                      const uint8_t* __restrict__ codes,
                      const uint8_t* __restrict__ scales,
                      const uint8_t* __restrict__ codes2,
                      const uint8_t* __restrict__ scales2,
                      const bf16_t* __restrict__ bias,
                      const bf16_t* __restrict__ res, bf16_t* __restrict__ y,
                      int M, int N, int K, int64_t ldx, int64_t ldc,
                      int64_t lds, int64_t ldc2, int64_t lds2, int64_t ldr,
                      int64_t ldy, int epi) {
  constexpr int T = DUAL ? 2 * RT : RT;  // weight tiles per K-step
  constexpr int F = T * MT;              // accumulator fragments per wave
  constexpr int U = skinny_mx::unroll(T, MT, BITS);
  constexpr int WQ = BITS / 4;           // 16-byte loads of one MX block
  constexpr int BLK = 4 * BITS;          // bytes of one MX block
  extern __shared__ f32x4 mx_part[];     // [NW][F][64 lanes]

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int NW = blockDim.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * RT);

  // this lane's weight rows (clamped to N - 1) at its block of a K-step,
  // and its token rows (clamped to M - 1) at the same 32 k
  const uint8_t* cp[T];
  const uint8_t* sp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int rt = DUAL ? t % RT : t;
    const int n = min(n0 + 16 * rt + i, N - 1);
    const bool second = DUAL && t >= RT;
    cp[t] = second ? codes2 + (int64_t)n * ldc2 + BLK * g
                   : codes + (int64_t)n * ldc + BLK * g;
    sp[t] = second ? scales2 + (int64_t)n * lds2 + g
                   : scales + (int64_t)n * lds + g;
  }
  const bf16_t* xp[MT];
  bool live[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = 16 * mt + i;
    live[mt] = m < M;
    xp[mt] = x + (int64_t)min(m, M - 1) * ldx + 32 * g;
  }

  f32x4 acc[T][MT];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the plan gives every wave at least one step: nj >= 1
  const int ksteps = K / skinny_mx::KSTEP;
  const int nj = (ksteps - wid + NW - 1) / NW;

  auto load = [&](int j0, u32x4 (&wr)[U][T][WQ], unsigned (&sr)[U][T],
                  u32x4 (&xr)[U][MT][4]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = min(j0 + u, nj - 1);  // past the end: the last step again
      const int step = wid + NW * j;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const uint8_t* c = cp[t] + (int64_t)step * (4 * BLK);
#pragma unroll
        for (int q = 0; q < WQ; ++q)
          wr[u][t][q] = *reinterpret_cast<const u32x4*>(c + 16 * q);
        sr[u][t] = sp[t][4 * step];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const bf16_t* xs = xp[mt] + (int64_t)step * skinny_mx::KSTEP;
#pragma unroll
        for (int d = 0; d < 4; ++d)
          xr[u][mt][d] = *reinterpret_cast<const u32x4*>(xs + 8 * d);
      }
    }
  };
  auto consume = [&](int j0, const u32x4 (&wr)[U][T][WQ],
                     const unsigned (&sr)[U][T],
                     const u32x4 (&xr)[U][MT][4]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j0 + u >= nj) break;  // wave-uniform
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        bf16x8 wf[T];  // dequantized once, used by every token fragment
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const float s = mx_scale(sr[u][t]);
          if constexpr (BITS == 4)
            wf[t] = dq_fp4(wr[u][t][0][d], s);
          else
            wf[t] = dq_fp8(wr[u][t][d / 2][2 * (d % 2)],
                           wr[u][t][d / 2][2 * (d % 2) + 1], s);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          u32x4 xv = xr[u][mt][d];
#pragma unroll
          for (int e = 0; e < 4; ++e) xv[e] = live[mt] ? xv[e] : 0u;
          const bf16x8 xb = __builtin_bit_cast(bf16x8, xv);
#pragma unroll
          for (int t = 0; t < T; ++t)
            acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[t], xb, acc[t][mt], 0, 0, 0);
        }
      }
    }
  };

  {
    u32x4 wa[U][T][WQ], xa[U][MT][4], wb[U][T][WQ], xb[U][MT][4];
    unsigned sa[U][T], sb[U][T];
    int j0 = 0;
    load(j0, wa, sa, xa);
    while (true) {
      load(j0 + U, wb, sb, xb);
      consume(j0, wa, sa, xa);
      j0 += U;
      if (j0 >= nj) break;
      load(j0 + U, wa, sa, xa);
      consume(j0, wb, sb, xb);
      j0 += U;
      if (j0 >= nj) break;
    }
  }

  // partial tiles to LDS: one 16-byte slot per (wave, fragment, lane)
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      mx_part[(wid * F + t * MT + mt) * WAVE + lane] = acc[t][mt];
  __syncthreads();

  // wave f % NW sums output fragment f = (rt, mt) over the waves in index
  // order and applies the epilogue
  const bool vec_y = (ldy & 3) == 0;
  const bool vec_r =
      (ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(res) & 7) == 0;
  for (int f = wid; f < RT * MT; f += NW) {
    const int rt = f / MT, mt = f % MT;
    f32x4 s = mx_part[(rt * MT + mt) * WAVE + lane];
    for (int ww = 1; ww < NW; ++ww) {
      const f32x4 p = mx_part[(ww * F + rt * MT + mt) * WAVE + lane];
      s += p;
    }
    float v[4] = {s[0], s[1], s[2], s[3]};
    if (DUAL) {
      f32x4 s2 = mx_part[((RT + rt) * MT + mt) * WAVE + lane];
      for (int ww = 1; ww < NW; ++ww) {
        const f32x4 p = mx_part[(ww * F + (RT + rt) * MT + mt) * WAVE + lane];
        s2 += p;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] * mx_sigmoid(v[e]) * s2[e];
    }
    const int m = 16 * mt + i;
    const int n = n0 + 16 * rt + 4 * g;
    if (m >= M || n >= N) continue;
    const bool whole = n + 3 < N;
    if (epi == SK_BIAS || epi == SK_BIAS_GELU || epi == SK_BIAS_RES) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += bf2f(bias[min(n + e, N - 1)]);
    }
    if (epi == SK_RES || epi == SK_BIAS_RES) {
      const bf16_t* rp = res + (int64_t)m * ldr + n;
      if (whole && vec_r) {  // 8-byte-aligned rows of r and n % 4 == 0
        const bf16x4 rv = *reinterpret_cast<const bf16x4*>(rp);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += bf2f(rv[e]);
      } else {
        for (int e = 0; e < 4 && n + e < N; ++e) v[e] += bf2f(rp[e]);
      }
    }
    if (epi == SK_BIAS_GELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gelu_f(v[e]);
    }
    bf16_t* yp = y + (int64_t)m * ldy + n;
    if (whole && vec_y) {
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
      *reinterpret_cast<bf16x4*>(yp) = o;
    } else {
      for (int e = 0; e < 4 && n + e < N; ++e) yp[e] = f2bf(v[e]);
    }
  }
}

// out[n][k .. k + 7] per thread: eight codes of one block, one 16-byte store
template <int BITS>
__global__ void mx_dequantize_kernel(const uint8_t* __restrict__ codes,
                                     const uint8_t* __restrict__ scales,
                                     bf16_t* __restrict__ out, int N, int K,
                                     int64_t ldc, int64_t lds, int64_t ldo) {
  const int k8 = K / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)N * k8) return;
  const int64_t n = idx / k8;
  const int k = (int)(idx % k8) * 8;
  const float s = mx_scale(scales[n * lds + k / 32]);
  bf16x8 v;
  if constexpr (BITS == 4) {
    v = dq_fp4(*reinterpret_cast<const unsigned*>(codes + n * ldc + k / 2), s);
  } else {
    const uint2 c = *reinterpret_cast<const uint2*>(codes + n * ldc + k);
    v = dq_fp8(c.x, c.y, s);
  }
  *reinterpret_cast<bf16x8*>(out + n * ldo + k) = v;
}

bool mx_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

template <int BITS, int MT, int RT, bool DUAL, typename... Args>
void mx_launch(const SkinnyMxPlan& p, int N, hipStream_t stream,
               Args... args) {
  constexpr int F = (DUAL ? 2 * RT : RT) * MT;
  const int blocks = (N + 16 * RT - 1) / (16 * RT);
  const size_t lds = (size_t)p.waves * F * WAVE * sizeof(f32x4);
  hipLaunchKernelGGL((skinny_mx_kernel<BITS, MT, RT, DUAL>), dim3(blocks),
                     dim3(p.waves * WAVE), lds, stream, args...);
}

}  // namespace

void skinny_mx_gemm(const void* x, const void* codes, const void* scales,
                    const void* codes2, const void* scales2, const void* bias,
                    const void* res, void* y, int M, int N, int K, int bits,
                    int64_t ldx, int64_t ldc, int64_t lds, int64_t ldc2,
                    int64_t lds2, int64_t ldr, int64_t ldy, int epi,
                    hipStream_t stream) {
  const bool dual = codes2 != nullptr;
  const SkinnyMxPlan p = skinny_mx_plan(M, N, K, bits, ldc, lds, epi, dual);
  if (p.why_not)
    throw std::runtime_error(std::string("skinny_mx_gemm: ") + p.why_not);
  const bool has_bias =
      epi == SK_BIAS || epi == SK_BIAS_GELU || epi == SK_BIAS_RES;
  const bool has_res = epi == SK_RES || epi == SK_BIAS_RES;
  if (!x || !codes || !scales || !y || dual != (scales2 != nullptr) ||
      has_bias != (bias != nullptr) || has_res != (res != nullptr))
    throw std::runtime_error("skinny_mx_gemm: operands do not match epi");
  if (!mx_aligned16(x) || ldx < K || (ldx & 7))
    throw std::runtime_error(
        "skinny_mx_gemm: x needs a 16-byte-aligned base and rows");
  if (!mx_aligned16(codes) || !mx_aligned16(codes2) ||
      (reinterpret_cast<uintptr_t>(scales) & 3) ||
      (reinterpret_cast<uintptr_t>(scales2) & 3))
    throw std::runtime_error(
        "skinny_mx_gemm: codes need a 16-byte-aligned base, scales a "
        "4-byte-aligned one");
  if (dual && skinny_mx_plan(M, N, K, bits, ldc2, lds2, epi, true).why_not)
    throw std::runtime_error(
        "skinny_mx_gemm: rows of the second weight are not aligned");
  if (has_res && ldr < N) throw std::runtime_error("skinny_mx_gemm: ldr < N");
  if (ldy < N) throw std::runtime_error("skinny_mx_gemm: ldy < N");

#define MX_GO(BB, MTT, RTT, DD)                                             \
  mx_launch<BB, MTT, RTT, DD>(                                              \
      p, N, stream, static_cast<const bf16_t*>(x),                          \
      static_cast<const uint8_t*>(codes),                                   \
      static_cast<const uint8_t*>(scales),                                  \
      static_cast<const uint8_t*>(codes2),                                  \
      static_cast<const uint8_t*>(scales2),                                 \
      static_cast<const bf16_t*>(bias), static_cast<const bf16_t*>(res),    \
      static_cast<bf16_t*>(y), M, N, K, ldx, ldc, lds, ldc2, lds2, ldr,     \
      ldy, epi)
#define MX_ROWS(BB, MTT)                                                    \
  do {                                                                      \
    if (dual) MX_GO(BB, MTT, 1, true);                                      \
    else if (p.rows == 32) MX_GO(BB, MTT, 2, false);                        \
    else MX_GO(BB, MTT, 1, false);                                          \
  } while (0)
#define MX_MT(BB)                                                           \
  switch (p.mt) {                                                           \
    case 1: MX_ROWS(BB, 1); break;                                          \
    case 2: MX_ROWS(BB, 2); break;                                          \
    default: MX_ROWS(BB, 4); break;                                         \
  }
  if (bits == 4) { MX_MT(4) } else { MX_MT(8) }
#undef MX_MT
#undef MX_ROWS
#undef MX_GO
}

void mx_dequantize_bf16(const void* codes, const void* scales, void* out,
                        int N, int K, int bits, int64_t ldc, int64_t lds,
                        int64_t ldo, hipStream_t stream) {
  if (bits != 4 && bits != 8)
    throw std::runtime_error("mx_dequantize: bits must be 4 or 8");
  if (N < 1 || K < 32 || K % 32 != 0)
    throw std::runtime_error(
        "mx_dequantize: N must be positive and K a positive multiple of 32");
  if (!codes || !scales || !out || !mx_aligned16(codes) ||
      !mx_aligned16(out) || ldc < (int64_t)K * bits / 8 || (ldc & 15) ||
      lds < K / 32 || ldo < K || (ldo & 7))
    throw std::runtime_error(
        "mx_dequantize: codes and out need 16-byte-aligned bases and rows "
        "of at least K elements, scales rows of at least K / 32");
  const int threads = 256;
  const int64_t total = (int64_t)N * (K / 8);
  const unsigned blocks = (unsigned)((total + threads - 1) / threads);
  const uint8_t* c = static_cast<const uint8_t*>(codes);
  const uint8_t* s = static_cast<const uint8_t*>(scales);
  bf16_t* o = static_cast<bf16_t*>(out);
  if (bits == 4)
    hipLaunchKernelGGL(mx_dequantize_kernel<4>, dim3(blocks), dim3(threads),
                       0, stream, c, s, o, N, K, ldc, lds, ldo);
  else
    hipLaunchKernelGGL(mx_dequantize_kernel<8>, dim3(blocks), dim3(threads),
                       0, stream, c, s, o, N, K, ldc, lds, ldo);
}

}  // namespace tepdist
