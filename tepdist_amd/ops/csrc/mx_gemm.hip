// LDS-tiled GEMM on OCP MX weights for gfx950:
//   y[M, N] = epi(x[M, K] . dq(W)[N, K]^T),  M >= 1, any N, K % 128 == 0,
//   x / bias / residual / y bf16, fp32 accumulate, one rounding,
// for the sites skinny_mx_gemm.hip does not take (M > 64: prefill, chunks,
// large decode batches). W is e2m1 or e4m3 codes with one e8m0 scale byte per
// 32 k of a row in the interchange layout of ops/mx.py; nothing is repacked,
// nothing is dequantized to memory. The result is defined like the skinny
// kernel's: the bf16 GEMM on the dequantized weight (an element times its
// power-of-two scale is exact in bf16). No split-K, no workspace, no atomics:
// every output is one wave's MFMA chain over K in order.
//
// Block and wave. 256 threads, 2 x 2 waves; wave (wm, wn) owns WM token
// fragments x WN weight fragments of mfma_f32_16x16x32_bf16 (weights are the
// A operand as in the skinny kernel, so a lane's four accumulator elements
// are four consecutive n of one token). Block tile (32 WM) x (32 WN): 128 x
// 128 (WM = WN = 4, 16 accumulator fragments) and 64 x 64 (WM = WN = 2).
//
// K-tile = 128 k, four MFMAs deep, in the skinny MX kernel's fragment order:
// lane 16g + i owns row i of a fragment and k 32g .. 32g + 31 of the tile,
// exactly one MX block and one scale byte; MFMA d takes k 32g + 8d .. + 7
// from both operands, so the k permutation inside a tile is free.
//
// LDS stage (three of them): three images, all staged by global_load_lds
// with the swizzle applied to the per-lane SOURCE address (the destination
// of a wave's DMA is lane-linear).
//  x       [BM][128] bf16, 256 B a row = 16 slots of 16 B. Slot s of row r
//          holds k 8 (s ^ (r & 15)). The fragment read of MFMA d is one
//          ds_read_b128 at slot (4g + d) ^ i of row 16 mt + i: the 16 lanes
//          of a group (g, d fixed) read 16 consecutive rows, whose slot
//          indices (4g + d) ^ i are the 16 different ones; a row is 64
//          banks wide, so the group covers every bank once. Unswizzled they
//          would share one slot: 16-way.
//  codes   [BN][RB] bytes as they lie, RB = 64 (e2m1) or 128 (e4m3) a row
//          and tile: 2 to 4 times smaller than a bf16 image. A lane reads
//          its whole MX block: one ds_read_b128 at slot g (e2m1, 4 slots a
//          row), two at slots 2g, 2g + 1 (e4m3, 8 slots a row). e2m1: four
//          rows fill the 64 banks, so rows i and i + 4 collide unswizzled;
//          slot s of row r holds bytes 16 (s ^ ((r >> 2) & 3)), and the 16
//          lanes of a group hit unit 4 (i & 3) + (g ^ (i >> 2)) of 16: all
//          different. e4m3: two rows fill the banks; slot s of row r holds
//          bytes 16 (s ^ ((r >> 1) & 7)), and for each of the two reads
//          (q = 0, 1) the group hits unit 8 (i & 1) + ((2g + q) ^ (i >> 1)):
//          all different. Each read of the pair is its own instruction, so
//          each needs to be conflict-free on its own, and is.
//  scales  [BN][4] bytes, the tile's scale dword of every row. Lane (i, g)
//          reads byte g of row 16 t + i: 16 consecutive dwords per group,
//          the four groups of a row share a dword (broadcast).
// Dequantization happens in registers when the fragment is used (dq_fp4 /
// dq_fp8 of mx_dequant.h, 16 conversions per weight fragment and K-tile); a
// dequantized fragment is reused over the wave's WM token fragments. The two
// waves that share a weight fragment each convert it.
//
// Pipeline. Per stage every wave issues the same OPS DMAs: BM / 16 of x,
// BN * RB / 4096 of codes and one 4-byte DMA of scales (64 rows a wave; where
// BN < 256 the waves cover the rows more than once and write the same bytes
// to the same place, so that every wave's count is the same). Tile t lives in
// stage t % 3. Loop iteration t:
//   wait    vmcnt(OPS) if tile t + 1 was staged, else vmcnt(0): DMAs retire
//           in order, so all of this wave's share of tile t has landed and
//           tile t + 1 stays in flight across the barrier;
//   barrier (raw s_barrier behind lgkmcnt(0)): every wave's share of tile t
//           has landed, and every wave has retired its reads of tile t - 1;
//   stage   tile t + 2 into stage (t + 2) % 3 = (t - 1) % 3, free by the
//           barrier just taken;
//   compute tile t.
// The prologue stages tiles 0 and 1. nk = 1: only tile 0 is staged, the wait
// is vmcnt(0). nk = 2: iteration 0 waits vmcnt(OPS) (tile 1 in flight),
// stages nothing; iteration 1 waits vmcnt(0). nk = 3: iteration 0 stages
// tile 2 into the untouched third stage. nk > 3: iteration 1 is the first to
// restage (tile 3 over tile 0), after the barrier that follows every wave's
// compute of tile 0. The last two iterations stage nothing; the last waits
// vmcnt(0). No vector-memory load other than the DMAs is issued before the
// epilogue, so the counts hold.
//
// Edges. Token rows >= M and weight rows >= N are staged from the clamped
// row (M - 1, N - 1) and dropped at the store; K is whole tiles. Nothing
// outside x[M, K], the code and scale rows of W, bias[N], r[M, N] and
// y[M, N] is touched.
//
// Epilogue. Bias, residual and gelu are applied in fp32 on the accumulator
// fragments exactly as in the skinny kernel, rounded once, and deposited as
// bf16x4 into a [BM][BN + 8] image over the drained stages (the 16-byte pad
// puts the 16 rows of a group 4 banks apart: 8-byte writes at the 2-way
// minimum of 512 bytes a wave); the block then stores the image row-major in
// 16-byte chunks (element by element at the ragged N edge, or where y's rows
// are not 16-byte aligned). Blocks are ordered by xcd_remap with the M tiles
// of one weight panel adjacent, so a panel is read by one XCD.

#include <stdexcept>
#include <string>

#include "common.h"
#include "gemm_tile.h"
#include "kernels.h"
#include "mx_dequant.h"
#include "mx_gemm_plan.h"

namespace tepdist {

namespace {

constexpr int MXG_THREADS = 256;

template <int N>
DEV_INLINE void mxg_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int BITS, int WM, int WN>
__launch_bounds__(MXG_THREADS) __global__
void mx_gemm_kernel(const bf16_t* __restrict__ x,
                    const uint8_t* __restrict__ codes,
                    const uint8_t* __restrict__ scales,
                    const bf16_t* __restrict__ bias,
                    const bf16_t* __restrict__ res, bf16_t* __restrict__ y,
                    int M, int N, int K, int64_t ldx, int64_t ldc,
                    int64_t lds, int64_t ldr, int64_t ldy, int epi) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int KT = mx_tiled::KTILE;
  constexpr int RB = 16 * BITS;          // code bytes of a row and K-tile
  constexpr int SL = RB / 16;            // 16-byte slots of a code row
  constexpr int WQ = BITS / 4;           // 16-byte reads of one MX block
  constexpr int XC = BM / 16;            // x DMAs per thread and stage
  constexpr int CC = BN * SL / MXG_THREADS;  // code DMAs
  constexpr int OPS = XC + CC + 1;       // DMAs per wave and stage
  constexpr int XB = BM * KT * 2, CB = BN * RB, SB = BN * 4;
  constexpr int STAGE = XB + CB + SB;
  constexpr int LDI = BN + 8;            // output image row, elements
  static_assert(BM * LDI * 2 <= mx_tiled::STAGES * STAGE, "image fits");
  static_assert(mx_tiled::STAGES == 3, "the loop below cycles three stages");
  __shared__ __attribute__((aligned(16))) uint8_t smem[3 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int wm = wid >> 1, wn = wid & 1;
  const int nbm = (M + BM - 1) / BM;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (tile % nbm) * BM, n0 = (tile / nbm) * BN;

  // staging sources. DMA c of an image covers its bytes 4096 c .. + 4095,
  // thread tid the 16 at 4096 c + 16 tid: a wave's 1 KiB is lane-linear.
  const bf16_t* xg[XC];
#pragma unroll
  for (int c = 0; c < XC; ++c) {
    const int row = (c * MXG_THREADS + tid) >> 4, slot = tid & 15;
    xg[c] = x + (int64_t)min(m0 + row, M - 1) * ldx + 8 * (slot ^ (row & 15));
  }
  const uint8_t* cg[CC];
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    const int row = (c * MXG_THREADS + tid) / SL, slot = tid % SL;
    const int sw = BITS == 4 ? (row >> 2) & 3 : (row >> 1) & 7;
    cg[c] = codes + (int64_t)min(n0 + row, N - 1) * ldc + 16 * (slot ^ sw);
  }
  const int srow0 = (wid * 64) % BN;     // wave-uniform
  const uint8_t* sg = scales + (int64_t)min(n0 + srow0 + lane, N - 1) * lds;

  auto stage = [&](int t, int slot) {
    uint8_t* st = smem + slot * STAGE + wid * 1024;  // wave-uniform
#pragma unroll
    for (int c = 0; c < XC; ++c)
      __builtin_amdgcn_global_load_lds((glds_src_t)(xg[c] + (int64_t)t * KT),
                                       (glds_dst_t)(st + c * 4096), 16, 0, 0);
#pragma unroll
    for (int c = 0; c < CC; ++c)
      __builtin_amdgcn_global_load_lds(
          (glds_src_t)(cg[c] + (int64_t)t * RB),
          (glds_dst_t)(st + XB + c * 4096), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(
        (glds_src_t)(sg + 4 * t),
        (glds_dst_t)(smem + slot * STAGE + XB + CB + srow0 * 4), 4, 0, 0);
  };

  f32x4 acc[WN][WM];
#pragma unroll
  for (int t = 0; t < WN; ++t)
#pragma unroll
    for (int mt = 0; mt < WM; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's fragment rows inside a stage
  const int xoff = (wm * 16 * WM + i) * (KT * 2);
  const int coff = XB + (wn * 16 * WN + i) * RB;
  const int soff = XB + CB + (wn * 16 * WN + i) * 4 + g;
  const int csw = BITS == 4 ? (i >> 2) & 3 : (i >> 1) & 7;

  auto compute = [&](int slot) {
    const uint8_t* st = smem + slot * STAGE;
    u32x4 wr[WN][WQ];
    float sc[WN];
#pragma unroll
    for (int t = 0; t < WN; ++t) {
#pragma unroll
      for (int q = 0; q < WQ; ++q)
        wr[t][q] = *reinterpret_cast<const u32x4*>(
            st + coff + t * 16 * RB + 16 * ((WQ * g + q) ^ csw));
      sc[t] = mx_scale(st[soff + t * 64]);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      bf16x8 xb[WM];
#pragma unroll
      for (int mt = 0; mt < WM; ++mt)
        xb[mt] = *reinterpret_cast<const bf16x8*>(
            st + xoff + mt * 16 * (KT * 2) + 16 * ((4 * g + d) ^ i));
#pragma unroll
      for (int t = 0; t < WN; ++t) {
        bf16x8 wf;  // dequantized once, used by every token fragment
        if constexpr (BITS == 4)
          wf = dq_fp4(wr[t][0][d], sc[t]);
        else
          wf = dq_fp8(wr[t][d / 2][2 * (d % 2)],
                      wr[t][d / 2][2 * (d % 2) + 1], sc[t]);
#pragma unroll
        for (int mt = 0; mt < WM; ++mt)
          acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wf, xb[mt], acc[t][mt], 0, 0, 0);
      }
    }
  };

  const int nk = K / KT;  // >= 1 by the plan
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  int cur = 0, nxt = 2;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) mxg_wait_vm<OPS>();
    else mxg_wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 2 < nk) stage(t + 2, nxt);
    compute(cur);
    cur = cur == 2 ? 0 : cur + 1;
    nxt = nxt == 2 ? 0 : nxt + 1;
  }
  // no DMA in flight (the last wait was vmcnt(0)); every wave's fragment
  // reads retire before the image overwrites the stages
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  bf16_t* img = reinterpret_cast<bf16_t*>(smem);  // [BM][LDI]
  const bool has_bias =
      epi == SK_BIAS || epi == SK_BIAS_GELU || epi == SK_BIAS_RES;
  const bool has_res = epi == SK_RES || epi == SK_BIAS_RES;
  const bool vec_r =
      (ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(res) & 7) == 0;
#pragma unroll
  for (int t = 0; t < WN; ++t) {
    const int nl = wn * 16 * WN + 16 * t + 4 * g, n = n0 + nl;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (has_bias) {
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = bf2f(bias[min(n + e, N - 1)]);
    }
#pragma unroll
    for (int mt = 0; mt < WM; ++mt) {
      const int ml = wm * 16 * WM + 16 * mt + i, m = m0 + ml;
      float v[4] = {acc[t][mt][0], acc[t][mt][1], acc[t][mt][2],
                    acc[t][mt][3]};
      if (has_bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += bv[e];
      }
      if (has_res && m < M && n < N) {
        const bf16_t* rp = res + (int64_t)m * ldr + n;
        if (n + 3 < N && vec_r) {  // 8-byte-aligned rows of r, n % 4 == 0
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
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
      *reinterpret_cast<bf16x4*>(img + ml * LDI + nl) = o;
    }
  }
  __syncthreads();

  const bool vec_y =
      (ldy & 7) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  constexpr int CPR = BN / 8;  // 16-byte chunks of an image row
#pragma unroll
  for (int c = tid; c < BM * CPR; c += MXG_THREADS) {
    const int ml = c / CPR, nl = (c % CPR) * 8;
    const int m = m0 + ml, n = n0 + nl;
    if (m >= M || n >= N) continue;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(img + ml * LDI + nl);
    bf16_t* yp = y + (int64_t)m * ldy + n;
    if (n + 7 < N && vec_y) {
      *reinterpret_cast<bf16x8*>(yp) = v;
    } else {
      for (int e = 0; e < 8 && n + e < N; ++e) yp[e] = v[e];
    }
  }
}

bool mxg_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace

void mx_gemm(const void* x, const void* codes, const void* scales,
             const void* bias, const void* res, void* y, int M, int N, int K,
             int bits, int64_t ldx, int64_t ldc, int64_t lds, int64_t ldr,
             int64_t ldy, int epi, int tile, hipStream_t stream) {
  const MxGemmPlan p = mx_gemm_plan(M, N, K, bits, ldc, lds, epi, tile);
  if (p.why_not)
    throw std::runtime_error(std::string("mx_gemm: ") + p.why_not);
  const bool has_bias =
      epi == SK_BIAS || epi == SK_BIAS_GELU || epi == SK_BIAS_RES;
  const bool has_res = epi == SK_RES || epi == SK_BIAS_RES;
  if (!x || !codes || !scales || !y || has_bias != (bias != nullptr) ||
      has_res != (res != nullptr))
    throw std::runtime_error("mx_gemm: operands do not match epi");
  if (!mxg_aligned16(x) || ldx < K || (ldx & 7))
    throw std::runtime_error(
        "mx_gemm: x needs a 16-byte-aligned base and rows");
  if (!mxg_aligned16(codes) || (reinterpret_cast<uintptr_t>(scales) & 3))
    throw std::runtime_error(
        "mx_gemm: codes need a 16-byte-aligned base, scales a 4-byte-aligned "
        "one");
  if (has_res && ldr < N) throw std::runtime_error("mx_gemm: ldr < N");
  if (ldy < N) throw std::runtime_error("mx_gemm: ldy < N");

#define MXG_GO(BB, WW)                                                      \
  hipLaunchKernelGGL((mx_gemm_kernel<BB, WW, WW>), dim3(p.blocks),          \
                     dim3(MXG_THREADS), 0, stream,                          \
                     static_cast<const bf16_t*>(x),                         \
                     static_cast<const uint8_t*>(codes),                    \
                     static_cast<const uint8_t*>(scales),                   \
                     static_cast<const bf16_t*>(bias),                      \
                     static_cast<const bf16_t*>(res),                       \
                     static_cast<bf16_t*>(y), M, N, K, ldx, ldc, lds, ldr,  \
                     ldy, epi)
  if (bits == 4) {
    if (p.tile == 128) MXG_GO(4, 4); else MXG_GO(4, 2);
  } else {
    if (p.tile == 128) MXG_GO(8, 4); else MXG_GO(8, 2);
  }
#undef MXG_GO
}

}  // namespace tepdist
