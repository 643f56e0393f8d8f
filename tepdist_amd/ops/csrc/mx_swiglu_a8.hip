// Fused SwiGLU gate/up GEMM on OCP MX weights and MX activations for gfx950,
// on the scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4:
//   h[M, I] = bf16(silu(G) * U),  G = dq(Xq)[M, K] . dq(Wg)[I, K]^T,
//                                 U = dq(Xq)[M, K] . dq(Wu)[I, K]^T,
//   M >= 1, any I, K % 128 == 0, the three format pairs of mx_gemm_a8.hip
//   (W e2m1 / e4m3 x X e4m3, W e2m1 x X e2m1), fp32 accumulate, silu(g) * u on
//   the fp32 accumulators, ONE rounding to bf16. h leaves either as bf16
//   [M, I] or quantized by the rule of ops/mx.py's mx_quantize(h, fmt): e4m3
//   or e2m1 codes plus one e8m0 scale byte per 32 hidden columns of a token
//   (needs I % 32 == 0), the activation layout mx_gemm_a8.hip reads as it is.
// G, U and (in the quantized form) the bf16 h never reach memory. No split-K,
// no workspace, no atomics: every output is one wave's MFMA chain over K in
// order, so the result is bit-reproducible and the launch capturable.
//
// Everything up to the epilogue follows mx_gemm_a8.hip, whose header holds
// the register layout of the instruction, the LDS images with their swizzles
// and the three-stage DMA pipeline with its wait counts; only the work split
// differs, and this header says how.
//
// Paired weight tile. A block owns BM tokens x BH hidden columns, and its
// weight code image holds 2 BH rows: the BH gate rows, then the BH up rows of
// the same hidden columns (hidden rows >= I staged from row I - 1, as token
// rows >= M from row M - 1). Large tile: BM 128, BH 64; small tile: BM 64, BH
// 32. That is 128 or 64 weight rows against 128 or 64 token rows, so the
// x-code image, the weight-code image, the scale image [2 BH + BM][4], the
// DMAs per wave and stage and the LDS bytes are those of mx_gemm_a8.hip's
// 128- and 64-tile for each format pair. The scale DMA of a wave still covers
// 64 consecutive rows of the scale image, each lane picking gate, up or token
// scales by its row.
//
// Wave split. 256 threads. Large tile: 2 x 2 waves, wave (wm, wn) owns 64
// tokens (four token fragments) x 32 hidden columns (two hidden fragments),
// and holds BOTH the gate and the up fragments of those columns: 2 + 2 weight
// fragments against 4 token fragments, 16 scaled MFMAs, 4 + 4 fragment reads
// per K-tile and 64 accumulator registers, the figures of mx_gemm_a8.hip's
// 128-tile. Small tile: 4 x 1 waves, each 16 tokens (one fragment) x all 32
// hidden columns, 4 MFMAs per K-tile. Weights are the A operand, so D is
// [n][m]: lane (i, g) holds in element e of hidden fragment t the hidden
// column 16 t + 4 g + e of token i, for gate and up alike. The gate and the
// up value of one (token, hidden) pair therefore sit in the same lane and the
// same accumulator element, and silu(g) * u needs no data movement.
//
// MX block per wave. One MX block of the output is 32 consecutive hidden
// columns of one token, exactly one wave's two hidden fragments at either
// tile: 2 fragments x 4 elements in a lane, and the lanes i, 16 + i, 32 + i,
// 48 + i. The block amax (the integer maximum of the 15 magnitude bits of the
// rounded bf16 values, as in mx_act_quant.hip) is the lane's maximum over its
// 8 values and two butterfly steps at lane distances 16 and 32.
// Cross-lane mechanism: __shfl_xor (ds_bpermute_b32), twice per token
// fragment. DPP cannot do it: row_shr / quad_perm stay inside a row of 16
// lanes and these steps cross rows. v_permlane32_swap would serve the
// distance-32 step and v_permlane16_swap the other, at a v_mov pair each to
// keep the swapped halves; with 2 steps per 16 MFMA chains of K / 128
// instructions the epilogue is nowhere near the critical path, and the
// bpermute form reads plainly and has no operand-tying rules to get wrong.
// It moves no data through LDS memory, so the drained stages are not
// involved.
//
// Quantizing epilogue. Scale byte and codes come from mxq_scale_byte /
// mxq_e4m3 / mxq_scale_byte4 / mxq_e2m1 of mx_gemm_a8_plan.h, the functions
// the quantizer kernel runs. e4m3: the lane's four hidden columns of a
// fragment are one dword; e2m1: two bytes, the even hidden column in the low
// nibble. They are deposited into an LDS code image [BM][BH * bits / 8 + 16]
// bytes over the drained stages (behind the same lgkmcnt(0) + barrier as the
// bf16 image): the 16 pad bytes make the row stride 20, 12 or 8 dwords, with
// which the 16 rows x 4 dwords of one deposit fall into different banks at
// the large tile. Lanes with g == 0 deposit the scale byte into [BM][BH / 32].
// After a barrier the block stores code rows in 16-byte chunks where the
// output code rows are 16-byte aligned, else in 8-byte chunks (the plan
// guarantees 8): 64 B (e4m3) or 32 B (e2m1) per token row at the large tile,
// half that at the small one; the scale bytes leave as single bytes. Token
// rows >= M and hidden blocks >= I are dropped here; I % 32 == 0, so no chunk
// straddles the edge.
//
// bf16 output: the same kernel with OBITS = 0 deposits bf16x4 into a
// [BM][BH + 8] image and stores it row-major in 16-byte chunks, element by
// element at a ragged I edge or where h's rows are not 16-byte aligned, as
// mx_gemm_a8.hip does.

#include <stdexcept>
#include <string>

#include "common.h"
#include "gemm_tile.h"
#include "kernels.h"
#include "mx_swiglu_a8_plan.h"

namespace tepdist {

namespace {

constexpr int MXS_THREADS = 256;

typedef int i32x8 __attribute__((ext_vector_type(8)));

template <int N>
DEV_INLINE void mxs_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The form of ops.swiglu's kernel (sigf of llama_ops.hip) and of the skinny
// dual kernels: g * sigmoid(g) is -0 for large negative finite g and NaN for
// g = -inf (-inf * 0), there as here.
DEV_INLINE float mxs_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

template <int BITS, int XBITS, bool BIG, int OBITS>
__launch_bounds__(MXS_THREADS) __global__
void mx_swiglu_a8_kernel(const uint8_t* __restrict__ xcodes,
                         const uint8_t* __restrict__ xscales,
                         const uint8_t* __restrict__ gcodes,
                         const uint8_t* __restrict__ gscales,
                         const uint8_t* __restrict__ ucodes,
                         const uint8_t* __restrict__ uscales,
                         bf16_t* __restrict__ y, uint8_t* __restrict__ ocodes,
                         uint8_t* __restrict__ oscales, int M, int I, int K,
                         int64_t ldxc, int64_t ldxs, int64_t ldc, int64_t lds,
                         int64_t ldy, int64_t ldoc, int64_t ldos) {
  static_assert(XBITS == 8 || (XBITS == 4 && BITS == 4), "W8A4 is not built");
  constexpr int WN = BIG ? 2 : 1;        // waves across the hidden columns
  constexpr int WM = BIG ? 4 : 1;        // token fragments of a wave
  constexpr int BM = 16 * WM * (4 / WN); // tokens of a block: 128 or 64
  constexpr int BH = 32 * WN;            // hidden columns: 64 or 32
  constexpr int WR = 2 * BH;             // weight rows: gate, then up
  constexpr int KT = mx_tiled::KTILE;    // k of a tile
  constexpr int RB = 16 * BITS;          // w code bytes of a row and K-tile
  constexpr int SL = RB / 16;            // 16-byte slots of a w code row
  constexpr int WQ = BITS / 4;           // 16-byte reads of one w MX block
  constexpr int XRB = 16 * XBITS;        // x code bytes of a row and K-tile
  constexpr int XSL = XRB / 16;          // 16-byte slots of an x code row
  constexpr int XQ = XBITS / 4;          // 16-byte reads of one x fragment
  constexpr int XC = BM * XSL / MXS_THREADS;  // x code DMAs per thread
  constexpr int CC = WR * SL / MXS_THREADS;   // w code DMAs
  constexpr int OPS = XC + CC + 1;       // DMAs per wave and stage
  constexpr int XB = BM * XRB, CB = WR * RB, SB = (WR + BM) * 4;
  constexpr int STAGE = XB + CB + SB;
  constexpr int LDI = BH + 8;            // bf16 image row, elements
  constexpr int ROWB = BH * OBITS / 8;   // output code bytes of a token row
  constexpr int CLD = ROWB + 16;         // code image row, bytes
  constexpr int SPR = BH / 32;           // scale bytes of a token row
  static_assert(BM * LDI * 2 <= mx_tiled::STAGES * STAGE, "image fits");
  static_assert(BM * (CLD + SPR) <= mx_tiled::STAGES * STAGE, "image fits");
  static_assert(mx_tiled::STAGES == 3, "the loop below cycles three stages");
  static_assert((WR + BM) % 64 == 0 && (WR + BM) / 64 <= 4,
                "a wave's scale DMA covers 64 rows of the scale image");
  __shared__ __attribute__((aligned(16))) uint8_t smem[3 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int wm = wid / WN, wn = wid % WN;
  const int nbm = (M + BM - 1) / BM;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (tile % nbm) * BM, h0 = (tile / nbm) * BH;

  // row r of the paired weight tile: gate row h0 + r, or up row h0 + r - BH
  auto wrow = [&](const uint8_t* gate, const uint8_t* up, int r, int64_t ld) {
    return (r < BH ? gate : up) + (int64_t)min(h0 + (r % BH), I - 1) * ld;
  };

  // staging sources, as in mx_gemm_a8.hip: DMA c of an image covers its
  // bytes 4096 c .. + 4095, thread tid the 16 at 4096 c + 16 tid
  const uint8_t* xg[XC];
#pragma unroll
  for (int c = 0; c < XC; ++c) {
    const int row = (c * MXS_THREADS + tid) / XSL, slot = tid % XSL;
    const int sw = XBITS == 4 ? (row >> 2) & 3 : (row >> 1) & 7;
    xg[c] = xcodes + (int64_t)min(m0 + row, M - 1) * ldxc + 16 * (slot ^ sw);
  }
  const uint8_t* cg[CC];
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    const int row = (c * MXS_THREADS + tid) / SL, slot = tid % SL;
    const int sw = BITS == 4 ? (row >> 2) & 3 : (row >> 1) & 7;
    cg[c] = wrow(gcodes, ucodes, row, ldc) + 16 * (slot ^ sw);
  }
  // scale image rows 0 .. WR - 1 are weight rows, WR .. WR + BM - 1 token
  // rows; this wave stages the 64 from srow0 (wave-uniform), lane by lane
  const int srow0 = (wid * 64) % (WR + BM), srow = srow0 + lane;
  const uint8_t* sg =
      srow < WR ? wrow(gscales, uscales, srow, lds)
                : xscales + (int64_t)min(m0 + srow - WR, M - 1) * ldxs;

  auto stage = [&](int t, int slot) {
    uint8_t* st = smem + slot * STAGE + wid * 1024;  // wave-uniform
#pragma unroll
    for (int c = 0; c < XC; ++c)
      __builtin_amdgcn_global_load_lds((glds_src_t)(xg[c] + (int64_t)t * XRB),
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

  // acc[f][mt]: f = 0, 1 the wave's two gate fragments, 2, 3 its up fragments
  f32x4 acc[4][WM];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int mt = 0; mt < WM; ++mt) acc[f][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's fragment rows inside a stage
  const int xoff = (wm * 16 * WM + i) * XRB;
  const int coff = XB + (wn * 32 + i) * RB;
  const int wsoff = XB + CB + (wn * 32 + i) * 4 + g;
  const int xsoff = XB + CB + (WR + wm * 16 * WM + i) * 4 + g;
  const int xsw = XBITS == 4 ? (i >> 2) & 3 : (i >> 1) & 7;
  const int csw = BITS == 4 ? (i >> 2) & 3 : (i >> 1) & 7;

  auto compute = [&](int slot) {
    const uint8_t* st = smem + slot * STAGE;
    i32x8 wf[4];
    int ws[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int row = (f >> 1) * BH + (f & 1) * 16;  // + wn * 32 + i
      u32x4 r[2] = {u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}};
#pragma unroll
      for (int q = 0; q < WQ; ++q)
        r[q] = *reinterpret_cast<const u32x4*>(
            st + coff + row * RB + 16 * ((g + 4 * q) ^ csw));
      wf[f] = i32x8{(int)r[0][0], (int)r[0][1], (int)r[0][2], (int)r[0][3],
                    (int)r[1][0], (int)r[1][1], (int)r[1][2], (int)r[1][3]};
      ws[f] = st[wsoff + row * 4];
    }
#pragma unroll
    for (int mt = 0; mt < WM; ++mt) {
      const uint8_t* xr = st + xoff + mt * 16 * XRB;
      u32x4 r[2] = {u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}};
#pragma unroll
      for (int q = 0; q < XQ; ++q)
        r[q] = *reinterpret_cast<const u32x4*>(xr + 16 * ((g + 4 * q) ^ xsw));
      const i32x8 xf = {(int)r[0][0], (int)r[0][1], (int)r[0][2], (int)r[0][3],
                        (int)r[1][0], (int)r[1][1], (int)r[1][2], (int)r[1][3]};
      const int xs = st[xsoff + mt * 64];
#pragma unroll
      for (int f = 0; f < 4; ++f)
        acc[f][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            wf[f], xf, acc[f][mt], BITS == 4 ? 4 : 0, XBITS == 4 ? 4 : 0, 0,
            ws[f], 0, xs);
    }
  };

  const int nk = K / KT;  // >= 1 by the plan
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  int cur = 0, nxt = 2;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) mxs_wait_vm<OPS>();
    else mxs_wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 2 < nk) stage(t + 2, nxt);
    compute(cur);
    cur = cur == 2 ? 0 : cur + 1;
    nxt = nxt == 2 ? 0 : nxt + 1;
  }
  // no DMA in flight (the last wait was vmcnt(0)); every wave's fragment
  // reads retire before an image overwrites the stages
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  if constexpr (OBITS == 0) {
    bf16_t* img = reinterpret_cast<bf16_t*>(smem);  // [BM][LDI]
#pragma unroll
    for (int mt = 0; mt < WM; ++mt) {
      const int ml = wm * 16 * WM + 16 * mt + i;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gv = acc[t][mt][e];
          o[e] = f2bf(gv * mxs_sigmoid(gv) * acc[2 + t][mt][e]);
        }
        *reinterpret_cast<bf16x4*>(img + ml * LDI + wn * 32 + 16 * t + 4 * g) =
            o;
      }
    }
    __syncthreads();

    const bool vec_y =
        (ldy & 7) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    constexpr int CPR = BH / 8;  // 16-byte chunks of an image row
#pragma unroll
    for (int c = tid; c < BM * CPR; c += MXS_THREADS) {
      const int ml = c / CPR, nl = (c % CPR) * 8;
      const int m = m0 + ml, n = h0 + nl;
      if (m >= M || n >= I) continue;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(img + ml * LDI + nl);
      bf16_t* yp = y + (int64_t)m * ldy + n;
      if (n + 7 < I && vec_y) {
        *reinterpret_cast<bf16x8*>(yp) = v;
      } else {
        for (int e = 0; e < 8 && n + e < I; ++e) yp[e] = v[e];
      }
    }
  } else {
    uint8_t* cimg = smem;               // [BM][CLD] code bytes
    uint8_t* simg = smem + BM * CLD;    // [BM][SPR] scale bytes
#pragma unroll
    for (int mt = 0; mt < WM; ++mt) {
      const int ml = wm * 16 * WM + 16 * mt + i;
      unsigned hb[2][4], amax = 0;      // bf16 patterns of the lane's 8 h
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gv = acc[t][mt][e];
          hb[t][e] = __builtin_bit_cast(
              unsigned short, f2bf(gv * mxs_sigmoid(gv) * acc[2 + t][mt][e]));
          amax = max(amax, hb[t][e] & 0x7fffu);
        }
      amax = max(amax, (unsigned)__shfl_xor((int)amax, 16, 64));
      amax = max(amax, (unsigned)__shfl_xor((int)amax, 32, 64));
      const unsigned byte =
          OBITS == 4 ? mxq_scale_byte4(amax) : mxq_scale_byte(amax);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        unsigned q = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          q |= (OBITS == 4 ? mxq_e2m1(hb[t][e], byte)
                           : mxq_e4m3(hb[t][e], byte)) << (OBITS * e);
        uint8_t* cp = cimg + ml * CLD + (wn * 32 + 16 * t + 4 * g) * OBITS / 8;
        if constexpr (OBITS == 4)
          *reinterpret_cast<unsigned short*>(cp) = (unsigned short)q;
        else
          *reinterpret_cast<unsigned*>(cp) = q;
      }
      if (g == 0) simg[ml * SPR + wn] = (uint8_t)byte;
    }
    __syncthreads();

    // whole MX blocks of this tile inside I (I % 32 == 0 by the plan)
    const int valid = min(BH, I - h0) * OBITS / 8;
    uint8_t* op = ocodes + (int64_t)h0 * OBITS / 8;
    auto store_rows = [&](auto chunk) {
      using V = decltype(chunk);
      constexpr int CPR = ROWB / (int)sizeof(V);
#pragma unroll
      for (int c = tid; c < BM * CPR; c += MXS_THREADS) {
        const int ml = c / CPR, off = (c % CPR) * (int)sizeof(V);
        if (m0 + ml >= M || off >= valid) continue;
        *reinterpret_cast<V*>(op + (int64_t)(m0 + ml) * ldoc + off) =
            *reinterpret_cast<const V*>(cimg + ml * CLD + off);
      }
    };
    if ((ldoc & 15) == 0 && (reinterpret_cast<uintptr_t>(ocodes) & 15) == 0)
      store_rows(u32x4{});
    else
      store_rows(uint2{});
    for (int c = tid; c < BM * SPR; c += MXS_THREADS) {
      const int ml = c / SPR, j = c % SPR;
      if (m0 + ml < M && h0 + 32 * j < I)
        oscales[(int64_t)(m0 + ml) * ldos + h0 / 32 + j] = simg[c];
    }
  }
}

}  // namespace

void mx_swiglu_a8(const void* xcodes, const void* xscales, const void* gcodes,
                  const void* gscales, const void* ucodes, const void* uscales,
                  void* y, void* ocodes, void* oscales, int M, int I, int K,
                  int bits, int64_t ldxc, int64_t ldxs, int64_t ldc,
                  int64_t lds, int64_t ldy, int64_t ldoc, int64_t ldos,
                  int tile, hipStream_t stream, int x_bits, int out_bits) {
  const MxGemmPlan p = mx_swiglu_a8_plan(
      M, I, K, bits, ldc, lds, I, K, bits, ldc, lds, ldxc, ldxs, SK_NONE, tile,
      x_bits, out_bits, ldoc, ldos);
  if (p.why_not)
    throw std::runtime_error(std::string("mx_swiglu_a8: ") + p.why_not);
  if (!xcodes || !xscales || !gcodes || !gscales || !ucodes || !uscales ||
      (out_bits == 0) != (y != nullptr) ||
      (out_bits != 0) != (ocodes != nullptr && oscales != nullptr))
    throw std::runtime_error("mx_swiglu_a8: operands do not match out_bits");
  auto a = [](const void* q, int n) {
    return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0;
  };
  if (!a(xcodes, 16) || !a(gcodes, 16) || !a(ucodes, 16) || !a(xscales, 4) ||
      !a(gscales, 4) || !a(uscales, 4))
    throw std::runtime_error(
        "mx_swiglu_a8: codes need a 16-byte-aligned base, scales a "
        "4-byte-aligned one");
  if (out_bits == 0 && ldy < I)
    throw std::runtime_error("mx_swiglu_a8: ldy < I");
  if (out_bits != 0 && !a(ocodes, 8))
    throw std::runtime_error(
        "mx_swiglu_a8: output codes need an 8-byte-aligned base");

#define MXS_GO(BB, XX, BIG, OO)                                             \
  hipLaunchKernelGGL((mx_swiglu_a8_kernel<BB, XX, BIG, OO>),                \
                     dim3(p.blocks), dim3(MXS_THREADS), 0, stream,          \
                     static_cast<const uint8_t*>(xcodes),                   \
                     static_cast<const uint8_t*>(xscales),                  \
                     static_cast<const uint8_t*>(gcodes),                   \
                     static_cast<const uint8_t*>(gscales),                  \
                     static_cast<const uint8_t*>(ucodes),                   \
                     static_cast<const uint8_t*>(uscales),                  \
                     static_cast<bf16_t*>(y), static_cast<uint8_t*>(ocodes),\
                     static_cast<uint8_t*>(oscales), M, I, K, ldxc, ldxs,   \
                     ldc, lds, ldy, ldoc, ldos)
#define MXS_OUT(BB, XX, BIG)                                                \
  do {                                                                      \
    if (out_bits == 0) MXS_GO(BB, XX, BIG, 0);                              \
    else if (out_bits == 8) MXS_GO(BB, XX, BIG, 8);                         \
    else MXS_GO(BB, XX, BIG, 4);                                            \
  } while (0)
#define MXS_TILE(BB, XX)                                                    \
  do {                                                                      \
    if (p.tile == 128) MXS_OUT(BB, XX, true); else MXS_OUT(BB, XX, false);  \
  } while (0)
  if (x_bits == 4) MXS_TILE(4, 4);  // the plan has refused it with e4m3 weights
  else if (bits == 4) MXS_TILE(4, 8);
  else MXS_TILE(8, 8);
#undef MXS_TILE
#undef MXS_OUT
#undef MXS_GO
}

}  // namespace tepdist
