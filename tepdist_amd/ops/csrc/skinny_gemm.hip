// Skinny-M weight-streaming GEMM for decode-step linears on gfx950:
//   y[M, N] = epi(x[M, K] . W[N, K]^T),  1 <= M <= 64, bf16 in, fp32
//   accumulate, bf16 out,
// and the dual form y = silu(x . Wg^T) * (x . Wu^T) in one launch.
//
// Every weight byte is used once and x is tiny, so the kernel is a weight
// stream, not a tile GEMM:
//
// * Weights are the MFMA A operand. mfma_f32_16x16x32_bf16 takes 16 weight
//   rows as its rows and 16 tokens as its columns; MT = 1, 2 or 4 token
//   fragments are multiplied against each weight fragment, so a fragment
//   fetched once from HBM serves up to 64 tokens. Token rows >= M are
//   zero-filled (the fragment is cleared in registers before the MFMA, the
//   load itself is clamped to row M - 1), never masked.
// * Weights go global -> VGPR in 16-byte loads and never touch LDS: no byte
//   is shared between waves. Lane 16g + i owns row i of a tile and, in a
//   K-step of 64, elements 16g .. 16g + 15: a contiguous 32-byte run, the
//   first half feeding the step's first MFMA and the second half the second
//   one. That permutes k inside the step; x fragments are read in the same
//   order, and the sum over k does not care. The four lanes of a row cover
//   one whole 128-byte line per step.
// * x is read straight from L2 in that same order, not from an LDS image:
//   at M = 64, K >= 2048 the image (256 KB and up) does not fit the 160 KB
//   LDS, and a staging pass would sit between launch and the first weight
//   load, where the kernel's time goes. A wave's x fragments of a K-step are
//   reused over every row tile the block owns (and both matrices when dual).
// * K is split inside the block: wave w owns K-steps w, w + NW, ... All
//   loads of U steps are issued before their first use, in two ping-pong
//   register sets with an unconditional clamped look-ahead (as in
//   decode_attention.hip), so a wave always has U to 2U steps in flight.
// * The waves' partial tiles are summed through LDS in wave order 0..NW-1,
//   fragment f by wave f % NW, then one epilogue on the fp32 sum with one
//   rounding. No atomics, no workspace: results repeat bit for bit.
// * The accumulator is a [16 n][16 m] tile and a lane holds 4 consecutive n
//   of one token: 8-byte stores along a row of y where N % 4 == 0, element
//   stores otherwise and in a ragged last tile; the residual is read the
//   same way (8-byte loads where its rows are 8-byte aligned). Weight loads
//   of a ragged tile are clamped to row N - 1.
//
// Grid-level split-K is not built (skinny_plan.h): the smallest flagship N
// (1024) still gives 64 blocks x 8 waves.

#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "skinny_plan.h"

namespace tepdist {

namespace {

constexpr int SK_MAX_THREADS = skinny::MAX_WAVES * WAVE;

DEV_INLINE float sk_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

DEV_INLINE bf16x8 as_frag(const uint4& u) {
  return __builtin_bit_cast(bf16x8, u);
}

// K-steps in flight per register set: S = 8 (T + MT) VGPRs per step
constexpr int sk_unroll(int T, int MT) {
  const int s = 8 * (T + MT);
  return s <= 24 ? 4 : s <= 40 ? 2 : 1;
}

template <int MT, int RT, bool DUAL>
__launch_bounds__(SK_MAX_THREADS) __global__
void skinny_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                   const bf16_t* __restrict__ w2,
                   const bf16_t* __restrict__ bias,
                   const bf16_t* __restrict__ res, bf16_t* __restrict__ y,
                   int M, int N, int K, int64_t ldx, int64_t ldw,
                   int64_t ldw2, int64_t ldr, int64_t ldy, int epi) {
  constexpr int T = DUAL ? 2 * RT : RT;  // weight tiles per K-step
  constexpr int F = T * MT;              // accumulator fragments per wave
  constexpr int U = sk_unroll(T, MT);
  extern __shared__ f32x4 sk_part[];     // [NW][F][64 lanes]

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int NW = blockDim.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * RT);

  // this lane's weight rows (clamped to N - 1) and token rows (clamped to
  // M - 1), at its 32-byte run of a K-step
  const bf16_t* wp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int rt = DUAL ? t % RT : t;
    const int n = min(n0 + 16 * rt + i, N - 1);
    wp[t] = (DUAL && t >= RT) ? w2 + (int64_t)n * ldw2 + 16 * g
                              : w + (int64_t)n * ldw + 16 * g;
  }
  const bf16_t* xp[MT];
  bool live[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = 16 * mt + i;
    live[mt] = m < M;
    xp[mt] = x + (int64_t)min(m, M - 1) * ldx + 16 * g;
  }

  f32x4 acc[T][MT];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the plan gives every wave at least one step: nj >= 1
  const int ksteps = K / skinny::KSTEP;
  const int nj = (ksteps - wid + NW - 1) / NW;

  auto load = [&](int j0, uint4 (&wr)[U][T][2], uint4 (&xr)[U][MT][2]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = min(j0 + u, nj - 1);  // past the end: the last step again
      const int k = (wid + NW * j) * skinny::KSTEP;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        wr[u][t][0] = *reinterpret_cast<const uint4*>(wp[t] + k);
        wr[u][t][1] = *reinterpret_cast<const uint4*>(wp[t] + k + 8);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        xr[u][mt][0] = *reinterpret_cast<const uint4*>(xp[mt] + k);
        xr[u][mt][1] = *reinterpret_cast<const uint4*>(xp[mt] + k + 8);
      }
    }
  };
  auto consume = [&](int j0, const uint4 (&wr)[U][T][2],
                     const uint4 (&xr)[U][MT][2]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j0 + u >= nj) break;  // wave-uniform
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          uint4 xv = xr[u][mt][kk];
          xv.x = live[mt] ? xv.x : 0u;
          xv.y = live[mt] ? xv.y : 0u;
          xv.z = live[mt] ? xv.z : 0u;
          xv.w = live[mt] ? xv.w : 0u;
          const bf16x8 xb = as_frag(xv);
#pragma unroll
          for (int t = 0; t < T; ++t)
            acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                as_frag(wr[u][t][kk]), xb, acc[t][mt], 0, 0, 0);
        }
      }
    }
  };

  {
    uint4 wa[U][T][2], xa[U][MT][2], wb[U][T][2], xb[U][MT][2];
    int j0 = 0;
    load(j0, wa, xa);
    while (true) {
      load(j0 + U, wb, xb);
      consume(j0, wa, xa);
      j0 += U;
      if (j0 >= nj) break;
      load(j0 + U, wa, xa);
      consume(j0, wb, xb);
      j0 += U;
      if (j0 >= nj) break;
    }
  }

  // partial tiles to LDS: one 16-byte slot per (wave, fragment, lane)
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      sk_part[(wid * F + t * MT + mt) * WAVE + lane] = acc[t][mt];
  __syncthreads();

  // wave f % NW sums output fragment f = (rt, mt) over the waves in index
  // order and applies the epilogue
  const bool vec_y = (ldy & 3) == 0;
  const bool vec_r =
      (ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(res) & 7) == 0;
  for (int f = wid; f < RT * MT; f += NW) {
    const int rt = f / MT, mt = f % MT;
    f32x4 s = sk_part[(rt * MT + mt) * WAVE + lane];
    for (int ww = 1; ww < NW; ++ww) {
      const f32x4 p = sk_part[(ww * F + rt * MT + mt) * WAVE + lane];
      s += p;
    }
    float v[4] = {s[0], s[1], s[2], s[3]};
    if (DUAL) {
      f32x4 s2 = sk_part[((RT + rt) * MT + mt) * WAVE + lane];
      for (int ww = 1; ww < NW; ++ww) {
        const f32x4 p = sk_part[(ww * F + (RT + rt) * MT + mt) * WAVE + lane];
        s2 += p;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] * sk_sigmoid(v[e]) * s2[e];
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

bool sk_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

template <int MT, int RT, bool DUAL>
void sk_launch(const SkinnyPlan& p, const bf16_t* x, const bf16_t* w,
               const bf16_t* w2, const bf16_t* bias, const bf16_t* res,
               bf16_t* y, int M, int N, int K, int64_t ldx, int64_t ldw,
               int64_t ldw2, int64_t ldr, int64_t ldy, int epi,
               hipStream_t stream) {
  constexpr int F = (DUAL ? 2 * RT : RT) * MT;
  const int blocks = (N + 16 * RT - 1) / (16 * RT);
  const size_t lds = (size_t)p.waves * F * WAVE * sizeof(f32x4);
  hipLaunchKernelGGL((skinny_kernel<MT, RT, DUAL>), dim3(blocks),
                     dim3(p.waves * WAVE), lds, stream, x, w, w2, bias, res,
                     y, M, N, K, ldx, ldw, ldw2, ldr, ldy, epi);
}

}  // namespace

void skinny_gemm_bf16(const void* x, const void* w, const void* w2,
                      const void* bias, const void* res, void* y, int M,
                      int N, int K, int64_t ldx, int64_t ldw, int64_t ldw2,
                      int64_t ldr, int64_t ldy, int epi, hipStream_t stream) {
  const bool dual = w2 != nullptr;
  const SkinnyPlan p = skinny_plan(M, N, K, ldx, ldw, epi, dual);
  if (p.why_not)
    throw std::runtime_error(std::string("skinny_gemm: ") + p.why_not);
  const bool has_bias =
      epi == SK_BIAS || epi == SK_BIAS_GELU || epi == SK_BIAS_RES;
  const bool has_res = epi == SK_RES || epi == SK_BIAS_RES;
  if (!x || !w || !y || has_bias != (bias != nullptr) ||
      has_res != (res != nullptr))
    throw std::runtime_error("skinny_gemm: operands do not match epi");
  if (!sk_aligned16(x) || !sk_aligned16(w) || !sk_aligned16(w2) ||
      (dual && (ldw2 < K || (ldw2 & 7))))
    throw std::runtime_error(
        "skinny_gemm: x and W need 16-byte-aligned bases and rows");
  if (has_res && ldr < N) throw std::runtime_error("skinny_gemm: ldr < N");
  if (ldy < N) throw std::runtime_error("skinny_gemm: ldy < N");

  const bf16_t* xp = static_cast<const bf16_t*>(x);
  const bf16_t* wp = static_cast<const bf16_t*>(w);
  const bf16_t* w2p = static_cast<const bf16_t*>(w2);
  const bf16_t* bp = static_cast<const bf16_t*>(bias);
  const bf16_t* rp = static_cast<const bf16_t*>(res);
  bf16_t* yp = static_cast<bf16_t*>(y);
#define SK_GO(MTT, RTT, DD)                                                 \
  sk_launch<MTT, RTT, DD>(p, xp, wp, w2p, bp, rp, yp, M, N, K, ldx, ldw,    \
                          ldw2, ldr, ldy, epi, stream)
#define SK_ROWS(MTT)                                                        \
  do {                                                                      \
    if (dual) SK_GO(MTT, 1, true);                                          \
    else if (p.rows == 32) SK_GO(MTT, 2, false);                            \
    else SK_GO(MTT, 1, false);                                              \
  } while (0)
  switch (p.mt) {
    case 1: SK_ROWS(1); break;
    case 2: SK_ROWS(2); break;
    default: SK_ROWS(4); break;
  }
#undef SK_ROWS
#undef SK_GO
}

}  // namespace tepdist
