// GEMM on OCP MX weights and MX activations for gfx950, on the scaled matrix
// instruction v_mfma_scale_f32_16x16x128_f8f6f4:
//   y[M, N] = epi(dq(Xq)[M, K] . dq(W)[N, K]^T),  M >= 1, any N, K % 128 == 0,
//   Xq e4m3 codes (W e2m1 or e4m3: W4A8, W8A8) or e2m1 codes (W e2m1 only:
//   W4A4, the instruction's double-rate form), one e8m0 scale byte per 32 k
//   of a row on both sides (the interchange layout of ops/mx.py, nothing repacked);
//   bias / residual / y bf16, fp32 accumulate, one rounding.
// Neither operand is ever dequantized: codes and scale bytes go from memory to
// LDS to the instruction's registers as they lie. No split-K, no workspace,
// no atomics: every output is one wave's MFMA chain over K in order.
//
// Block and wave. 256 threads, 2 x 2 waves; wave (wm, wn) owns WM token
// fragments x WN weight fragments. Weights are the A operand (cbsz 4 = e2m1
// or 0 = e4m3), activations B (blgp 0 = e4m3 or 4 = e2m1), so D is [n][m] and a lane's four
// accumulator elements are four consecutive n of one token, as in mx_gemm.hip
// and the skinny kernels. Block tile (32 WM) x (32 WN): 128 x 128 and 64 x 64.
//
// K-tile = 128 k = ONE instruction per (weight fragment, token fragment).
// The register layout was settled on the device by one-hot probes (the
// placement test holds it), and it differs by element width. e4m3, 8 VGPRs:
// lane 16 g + i holds row i, k 16 g .. 16 g + 15 in V0-3 and k 64 + 16 g ..
// 64 + 16 g + 15 in V4-7 (the instruction is two passes of 64 k). e2m1, 4
// VGPRs (the upper four are not read under cbsz 4): lane 16 g + i holds row
// i, k 32 g .. 32 g + 31. The B operand under blgp 4 mirrors the A operand
// under cbsz 4, lane map, nibble order (even k low) and scale lane alike: the
// one-hot placement test of the a4 suite was run on the device against this
// assumption and holds it. Scales, either width: the scale of row i and MX
// block b (k 32 b .. 32 b + 31) is the low byte of lane 16 b + i's scale
// VGPR (op_sel 0 on both sides); for e4m3 that lane holds only half of the
// block's elements, which is of no concern to the code: each lane reads the
// scale byte g of its row.
//
// LDS stage (three of them), every image staged by global_load_lds with the
// swizzle applied to the per-lane SOURCE address (the destination of a wave's
// DMA is lane-linear):
//  x codes, e2m1: [BM][64] bytes, the image, rule and single read of the
//          e2m1 weight rows below (four rows fill the banks, slot s of row r
//          holds bytes 16 (s ^ ((r >> 2) & 3)), the fragment is one
//          ds_read_b128 at slot g ^ (i >> 2) of row 16 mt + i, and the 16
//          lanes of a group hit unit 4 (i & 3) + (g ^ (i >> 2)) of the 16
//          units of the bank row: i & 3 picks the quarter, and within a
//          quarter i >> 2 runs over 0 .. 3, so g ^ (i >> 2) does: all
//          different). DMA rows are 64 B, four lanes a row.
//  x codes, e4m3: [BM][128] bytes, 8 slots of 16 B a row. Two rows fill the 64
//          banks, so rows i and i + 2 collide unswizzled; slot s of row r
//          holds bytes 16 (s ^ ((r >> 1) & 7)). A fragment is two
//          ds_read_b128 (q = 0, 1) at slots (g + 4 q) ^ (i >> 1) of row 16 mt
//          + i: for each read the 16 lanes of a group (g fixed) hit unit
//          8 (i & 1) + ((g + 4 q) ^ (i >> 1)) of the 16 16-byte units of the
//          bank row: all different.
//  w codes [BN][RB] bytes, RB = 64 (e2m1) or 128 (e4m3). e4m3: the rule and
//          the two reads above. e2m1: four rows fill the banks, slot s of row
//          r holds bytes 16 (s ^ ((r >> 2) & 3)); one ds_read_b128 at slot g
//          ^ (i >> 2), the group hits unit 4 (i & 3) + (g ^ (i >> 2)): all
//          different.
//  scales  [BN + BM][4] bytes: the tile's scale dword of every weight row,
//          then of every token row. Lane (i, g) reads byte g of its row with
//          one ds_read_u8: 16 consecutive dwords per group, 16 different
//          banks; the four groups of a row share a dword (broadcast).
// A stage is 33 KiB at 128 / e4m3 (25 KiB e2m1), 16.5 KiB at 64 (12.5 KiB):
// 99 of the 160 KiB at the 128-tile, three blocks per CU at the 64-tile. With
// e2m1 on both sides it is 17 KiB at 128 and 8.5 KiB at 64: 51 KiB, three
// blocks per CU at the 128-tile.
//
// K-tile of the e2m1 x e2m1 form: 128 k, three stages, the loop below as it
// is, so one barrier per WM * WN half-length MFMAs and 64-byte DMA rows. A
// 256-k tile (two instructions per fragment pair and stage, a tail stage for
// odd K / 128) would halve both counts per MFMA; it is not built, and the
// documentation lists it as not measured.
//
// Pipeline (the protocol of mx_gemm.hip). Per stage every wave issues the
// same OPS DMAs: BM * XRB / 4096 of x codes (XRB = 128 or 64), BN * RB / 4096 of w codes and one 4-byte
// DMA of scales: 64 rows a wave out of the BN + BM; at 128 waves 0, 1 take
// the weight rows and 2, 3 the token rows, at 64 waves 0 and 2 both take the
// weight rows and 1 and 3 the token rows (the same bytes to the same place,
// so that every wave's count is the same). Tile t lives in stage t % 3. Loop
// iteration t:
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
// outside the code and scale rows of Xq and W, bias[N], r[M, N] and y[M, N]
// is touched.
//
// Epilogue, as mx_gemm.hip's. Bias, residual and gelu in fp32 on the
// accumulator fragments, rounded once, deposited as bf16x4 into a [BM][BN +
// 8] image over the drained stages; the block then stores the image row-major
// in 16-byte chunks (element by element at the ragged N edge, or where y's
// rows are not 16-byte aligned). Blocks are ordered by xcd_remap with the M
// tiles of one weight panel adjacent, so a panel is read by one XCD.

#include <stdexcept>
#include <string>

#include "common.h"
#include "gemm_tile.h"
#include "kernels.h"
#include "mx_gemm_a8_plan.h"

namespace tepdist {

namespace {

constexpr int MXA_THREADS = 256;

typedef int i32x8 __attribute__((ext_vector_type(8)));

template <int N>
DEV_INLINE void mxa_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int BITS, int XBITS, int WM, int WN>
__launch_bounds__(MXA_THREADS) __global__
void mx_gemm_a8_kernel(const uint8_t* __restrict__ xcodes,
                       const uint8_t* __restrict__ xscales,
                       const uint8_t* __restrict__ codes,
                       const uint8_t* __restrict__ scales,
                       const bf16_t* __restrict__ bias,
                       const bf16_t* __restrict__ res, bf16_t* __restrict__ y,
                       int M, int N, int K, int64_t ldxc, int64_t ldxs,
                       int64_t ldc, int64_t lds, int64_t ldr, int64_t ldy,
                       int epi) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  static_assert(XBITS == 8 || (XBITS == 4 && BITS == 4), "W8A4 is not built");
  constexpr int KT = mx_tiled::KTILE;    // k of a tile
  constexpr int RB = 16 * BITS;          // w code bytes of a row and K-tile
  constexpr int SL = RB / 16;            // 16-byte slots of a w code row
  constexpr int WQ = BITS / 4;           // 16-byte reads of one w MX block
  constexpr int XRB = 16 * XBITS;        // x code bytes of a row and K-tile
  constexpr int XSL = XRB / 16;          // 16-byte slots of an x code row
  constexpr int XQ = XBITS / 4;          // 16-byte reads of one x fragment
  constexpr int XC = BM * XSL / MXA_THREADS;  // x code DMAs per thread
  constexpr int CC = BN * SL / MXA_THREADS;   // w code DMAs
  constexpr int OPS = XC + CC + 1;       // DMAs per wave and stage
  constexpr int XB = BM * XRB, CB = BN * RB, SB = (BN + BM) * 4;
  constexpr int STAGE = XB + CB + SB;
  constexpr int LDI = BN + 8;            // output image row, elements
  static_assert(BM * LDI * 2 <= mx_tiled::STAGES * STAGE, "image fits");
  static_assert(mx_tiled::STAGES == 3, "the loop below cycles three stages");
  static_assert(BM == BN, "the scale DMA below splits BN + BM rows by BN");
  __shared__ __attribute__((aligned(16))) uint8_t smem[3 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int wm = wid >> 1, wn = wid & 1;
  const int nbm = (M + BM - 1) / BM;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (tile % nbm) * BM, n0 = (tile / nbm) * BN;

  // staging sources. DMA c of an image covers its bytes 4096 c .. + 4095,
  // thread tid the 16 at 4096 c + 16 tid: a wave's 1 KiB is lane-linear.
  const uint8_t* xg[XC];
#pragma unroll
  for (int c = 0; c < XC; ++c) {
    const int row = (c * MXA_THREADS + tid) / XSL, slot = tid % XSL;
    const int sw = XBITS == 4 ? (row >> 2) & 3 : (row >> 1) & 7;
    xg[c] = xcodes + (int64_t)min(m0 + row, M - 1) * ldxc + 16 * (slot ^ sw);
  }
  const uint8_t* cg[CC];
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    const int row = (c * MXA_THREADS + tid) / SL, slot = tid % SL;
    const int sw = BITS == 4 ? (row >> 2) & 3 : (row >> 1) & 7;
    cg[c] = codes + (int64_t)min(n0 + row, N - 1) * ldc + 16 * (slot ^ sw);
  }
  // scale image rows 0 .. BN - 1 are weight rows, BN .. BN + BM - 1 token
  // rows; this wave stages the 64 from srow0 (wave-uniform)
  const int srow0 = (wid * 64) % (BN + BM);
  const uint8_t* sg =
      srow0 < BN
          ? scales + (int64_t)min(n0 + srow0 + lane, N - 1) * lds
          : xscales + (int64_t)min(m0 + srow0 - BN + lane, M - 1) * ldxs;

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

  f32x4 acc[WN][WM];
#pragma unroll
  for (int t = 0; t < WN; ++t)
#pragma unroll
    for (int mt = 0; mt < WM; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's fragment rows inside a stage
  const int xoff = (wm * 16 * WM + i) * XRB;
  const int coff = XB + (wn * 16 * WN + i) * RB;
  const int wsoff = XB + CB + (wn * 16 * WN + i) * 4 + g;
  const int xsoff = XB + CB + (BN + wm * 16 * WM + i) * 4 + g;
  const int xsw = XBITS == 4 ? (i >> 2) & 3 : (i >> 1) & 7;
  const int csw = BITS == 4 ? (i >> 2) & 3 : (i >> 1) & 7;

  auto compute = [&](int slot) {
    const uint8_t* st = smem + slot * STAGE;
    i32x8 wf[WN];
    int ws[WN];
#pragma unroll
    for (int t = 0; t < WN; ++t) {
      u32x4 r[2] = {u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}};
#pragma unroll
      for (int q = 0; q < WQ; ++q)
        r[q] = *reinterpret_cast<const u32x4*>(
            st + coff + t * 16 * RB + 16 * ((g + 4 * q) ^ csw));
      wf[t] = i32x8{(int)r[0][0], (int)r[0][1], (int)r[0][2], (int)r[0][3],
                    (int)r[1][0], (int)r[1][1], (int)r[1][2], (int)r[1][3]};
      ws[t] = st[wsoff + t * 64];
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
      for (int t = 0; t < WN; ++t)
        acc[t][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            wf[t], xf, acc[t][mt], BITS == 4 ? 4 : 0, XBITS == 4 ? 4 : 0, 0,
            ws[t], 0, xs);
    }
  };

  const int nk = K / KT;  // >= 1 by the plan
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  int cur = 0, nxt = 2;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) mxa_wait_vm<OPS>();
    else mxa_wait_vm<0>();
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
  for (int c = tid; c < BM * CPR; c += MXA_THREADS) {
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

}  // namespace

void mx_gemm_a8(const void* xcodes, const void* xscales, const void* codes,
                const void* scales, const void* bias, const void* res,
                void* y, int M, int N, int K, int bits, int64_t ldxc,
                int64_t ldxs, int64_t ldc, int64_t lds, int64_t ldr,
                int64_t ldy, int epi, int tile, hipStream_t stream,
                int x_bits) {
  const MxGemmPlan p =
      mx_gemm_a8_plan(M, N, K, bits, ldc, lds, ldxc, ldxs, epi, tile, x_bits);
  if (p.why_not)
    throw std::runtime_error(std::string("mx_gemm_a8: ") + p.why_not);
  const bool has_bias =
      epi == SK_BIAS || epi == SK_BIAS_GELU || epi == SK_BIAS_RES;
  const bool has_res = epi == SK_RES || epi == SK_BIAS_RES;
  if (!xcodes || !xscales || !codes || !scales || !y ||
      has_bias != (bias != nullptr) || has_res != (res != nullptr))
    throw std::runtime_error("mx_gemm_a8: operands do not match epi");
  auto a = [](const void* q, int n) {
    return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0;
  };
  if (!a(xcodes, 16) || !a(codes, 16) || !a(xscales, 4) || !a(scales, 4))
    throw std::runtime_error(
        "mx_gemm_a8: codes need a 16-byte-aligned base, scales a "
        "4-byte-aligned one");
  if (has_res && ldr < N) throw std::runtime_error("mx_gemm_a8: ldr < N");
  if (ldy < N) throw std::runtime_error("mx_gemm_a8: ldy < N");

#define MXA_GO(BB, XX, WW)                                                  \
  hipLaunchKernelGGL((mx_gemm_a8_kernel<BB, XX, WW, WW>), dim3(p.blocks),   \
                     dim3(MXA_THREADS), 0, stream,                          \
                     static_cast<const uint8_t*>(xcodes),                   \
                     static_cast<const uint8_t*>(xscales),                  \
                     static_cast<const uint8_t*>(codes),                    \
                     static_cast<const uint8_t*>(scales),                   \
                     static_cast<const bf16_t*>(bias),                      \
                     static_cast<const bf16_t*>(res),                       \
                     static_cast<bf16_t*>(y), M, N, K, ldxc, ldxs, ldc,     \
                     lds, ldr, ldy, epi)
  if (x_bits == 4) {  // the plan has refused it with e4m3 weights
    if (p.tile == 128) MXA_GO(4, 4, 4); else MXA_GO(4, 4, 2);
  } else if (bits == 4) {
    if (p.tile == 128) MXA_GO(4, 8, 4); else MXA_GO(4, 8, 2);
  } else {
    if (p.tile == 128) MXA_GO(8, 8, 4); else MXA_GO(8, 8, 2);
  }
#undef MXA_GO
}

}  // namespace tepdist
