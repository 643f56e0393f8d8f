// bf16 MFMA GEMM for gfx950 (MI355X), fp32 accumulation.
//
// Structure: 128x128 tile, BK=32, 4 waves per block (2x2 wave grid, 64x64
// per wave as 4x4 fragments of 16x16), double-buffered LDS with the
// load-early/write-late split (guide T14), mfma_f32_16x16x32_bf16 inner loop.
//
// Layout handling: both operands stage into the canonical k-contiguous
// row-padded [F][BK] LDS image (ds_read_b128 fragment reads, one row per
// lane in a 16-lane group; the +16B row pad keeps them bank-conflict-free).
//  - "KC" operands (k fastest-varying in memory: A stored [M,K], B stored
//    [N,K]): straight 16B loads + 16B LDS writes.
//  - "KO" operands (k outermost: stored [K,F] — dgrad's weight and both
//    wgrad operands): each thread loads an 8(k) x 2(f) slab with eight 4B
//    loads (f-coalesced across the wave), transposes it in registers with
//    eight v_perm_b32, and writes two k-contiguous 16B rows. No scalar LDS
//    traffic. (ds_read_b64_tr_b16 could form these fragments at read time
//    from the natural [K][F] image instead: per 16-lane group, lane 4q+p
//    supplies the 8B-aligned address of row q, columns 4p..4p+3 of a
//    4-row x 16-column block and lane i receives column i of the four rows
//    — two such reads make one 16x16x32 fragment, as tr_frag in lds_frag.h
//    does for the flash kernels. The first probe here, debug.hip tr16_probe,
//    addressed it as element lane&15 of row lane>>4; those unaligned
//    addresses collapse to the quad leaders' 8B words, which is why it saw
//    only 16 distinct values per group and this path took the register
//    transpose. The 256 kernel now reads two k-outer operands that way,
//    gemm256.hip; this kernel keeps the register transpose, which also
//    serves mixed layouts, partial tiles and unaligned rows.)
//
// Replaces the reference's XLA-codegen GEMMs (all device code
// in TePDist is XLA-generated PTX; here it is hand-written CDNA4).

#include <algorithm>
#include <stdexcept>
#include <string>

#include "common.h"
#include "gemm_tile.h"
#include "kernels.h"

namespace tepdist {

namespace {

constexpr int BM = plan::T128, BN = plan::T128, BK = plan::BK;
constexpr int SLOT = BM * BK;  // elements per operand slot
constexpr int NTHREADS = 256;

// LDS image: unpadded 128B rows, 16B column slots swizzled (lds_frag.h).
DEV_INLINE int lds_off(int row, int col_e) { return loff<BK>(row, col_e); }

// --- staging loads ---------------------------------------------------------

// KC operand (stored [F][ld], k inner): 2 x 16B per thread.
DEV_INLINE void stage_kc_load(const bf16_t* __restrict__ src, int F, int K,
                              int ld, int f0, int k0, bool aligned,
                              bf16x8 regs[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = threadIdx.x + u * NTHREADS;  // 0..1023
    const int row = idx >> 3;                    // 0..127
    const int kc = (idx & 7) * 8;
    bf16x8 v = {};
    const int f = f0 + row, k = k0 + kc;
    if (f < F && k < K) {
      const bf16_t* p = src + (int64_t)f * ld + k;
      if (aligned && k + 8 <= K) {
        v = *reinterpret_cast<const bf16x8*>(p);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (k + e < K) v[e] = p[e];
      }
    }
    regs[u] = v;
  }
}

// KO operand (stored [K][ld], f inner): thread t owns the 8(k) x 2(f) slab
// at f = 2*(t&63), k-block = t>>6; eight bf16x2 loads, f-coalesced.
DEV_INLINE void stage_ko_load(const bf16_t* __restrict__ src, int F, int K,
                              int ld, int f0, int k0, bool aligned,
                              bf16x2 regs[2][8]) {
  const int f = f0 + 2 * (threadIdx.x & 63);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int kt = k0 + 8 * ((threadIdx.x >> 6) + 4 * h);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = kt + j;
      bf16x2 v = {};
      if (k < K && f < F) {
        const bf16_t* p = src + (int64_t)k * ld + f;
        if (aligned && f + 2 <= F) {
          v = *reinterpret_cast<const bf16x2*>(p);
        } else {
          v[0] = p[0];
          if (f + 1 < F) v[1] = p[1];
        }
      }
      regs[h][j] = v;
    }
  }
}

// KC operand via global_load_lds (direct HBM->LDS DMA, 16B per lane; the
// guide's step-3 lever), swizzle on the source address (gemm_tile.h).
// Only for fully-interior tiles (no bounds handling in the DMA).
DEV_INLINE void stage_kc_glds(const bf16_t* __restrict__ src, int ld, int f0,
                              int k0, bf16_t* dst) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = threadIdx.x + u * NTHREADS;
    const int row = idx >> 3;                 // dest row (lane-linear)
    const int c = (idx & 7) * 8;              // dest column (elements)
    const int ksrc = k0 + (c ^ (SWZ8(row) << 3));  // inverse swizzle
    const bf16_t* g = src + (int64_t)(f0 + row) * ld + ksrc;
    bf16_t* l = dst + (8 * wave + 32 * u) * BK;  // wave-uniform base
    __builtin_amdgcn_global_load_lds((glds_src_t)g, (glds_dst_t)l, 16,
                                     /*offset=*/0, /*aux=*/0);
  }
}

// --- staging writes --------------------------------------------------------

// natural k order (used when both operands are KC)
DEV_INLINE void stage_write_kc_natural(bf16_t* dst, const bf16x8 regs[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = threadIdx.x + u * NTHREADS;
    const int row = idx >> 3;
    const int kc = (idx & 7) * 8;
    *reinterpret_cast<bf16x8*>(dst + lds_off(row, kc)) = regs[u];
  }
}

// KO slab write: transpose 8x2 in registers (v_perm_b32), two b128 writes.
DEV_INLINE void stage_write_ko(bf16_t* dst, const bf16x2 regs[2][8]) {
  const int f = 2 * (threadIdx.x & 63);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int kc = 8 * ((threadIdx.x >> 6) + 4 * h);
    uint32_t r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      r[j] = __builtin_bit_cast(uint32_t, regs[h][j]);
    uint32_t o0[4], o1[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      // result bytes [A0,A1,B0,B1]: A=r[2d] (src1=bytes 0-3), B=r[2d+1]
      o0[d] = __builtin_amdgcn_perm(r[2 * d + 1], r[2 * d], 0x05040100u);
      o1[d] = __builtin_amdgcn_perm(r[2 * d + 1], r[2 * d], 0x07060302u);
    }
    *reinterpret_cast<uint4*>(dst + lds_off(f, kc)) =
        make_uint4(o0[0], o0[1], o0[2], o0[3]);
    *reinterpret_cast<uint4*>(dst + lds_off(f + 1, kc)) =
        make_uint4(o1[0], o1[1], o1[2], o1[3]);
  }
}

// --- fragment loads --------------------------------------------------------

// fragment read from the canonical [F][LDS_ROW] image
DEV_INLINE bf16x8 frag(const bf16_t* s, int fbase, int lane, int kk) {
  return *reinterpret_cast<const bf16x8*>(
      s + lds_off(fbase + (lane & 15), 8 * (lane >> 4) + 32 * kk));
}

// F32OUT: split-K mode — blockIdx.z selects a K-chunk (k_chunk elements)
// of batch-0 operands and the epilogue writes fp32 partials at
// C + z*strideC (reduced by splitk_reduce_kernel).
template <bool A_KC, bool B_KC, int EPI, bool F32OUT = false>
__launch_bounds__(NTHREADS) __global__
void gemm_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                 void* __restrict__ Cv, bf16_t* __restrict__ Cpre,
                 const bf16_t* __restrict__ bias, int M, int N, int K,
                 int lda, int ldb, int ldc, int64_t strideA, int64_t strideB,
                 int64_t strideC, int k_chunk) {
  bf16_t* C = static_cast<bf16_t*>(Cv);
  float* Cf = static_cast<float*>(Cv);
  int kbeg = 0, kend = K;
  if (F32OUT) {
    kbeg = blockIdx.z * k_chunk;
    kend = min(K, kbeg + k_chunk);
    Cf += blockIdx.z * strideC;
  } else {
    A += blockIdx.z * strideA;
    B += blockIdx.z * strideB;
    C += blockIdx.z * strideC;
    if (EPI >= 2) Cpre += blockIdx.z * strideC;
  }

  const int nbx = (N + BN - 1) / BN;
  const int swz = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (swz / nbx) * BM, n0 = (swz % nbx) * BN;

  __shared__ bf16_t smem[2][2][SLOT];  // [buf][A=0/B=1]

  const int lane = threadIdx.x & 63;
  const int wm = (threadIdx.x >> 7) * 64;        // wave row (wid>>1)*64
  const int wn = ((threadIdx.x >> 6) & 1) * 64;  // wave col (wid&1)*64

  const bool a_al = (lda & 7) == 0;   // 16B loads (KC staging)
  const bool b_al = (ldb & 7) == 0;
  const bool a_al2 = (lda & 1) == 0;  // 4B loads (KO staging)
  const bool b_al2 = (ldb & 1) == 0;

  f32x4 acc[4][4] = {};

  const int nk = (kend - kbeg + BK - 1) / BK;
  bf16x8 ra_kc[4], rb_kc[4];
  bf16x2 ra_ko[2][8], rb_ko[2][8];

  // interior tiles of aligned KC operands go by global_load_lds DMA
  const bool a_glds = A_KC && a_al && (m0 + BM <= M);
  const bool b_glds = B_KC && b_al && (n0 + BN <= N);

  auto load_tiles = [&](int k0, int buf) {
    const bool kin = k0 + BK <= kend;
    if (A_KC) {
      if (a_glds && kin) stage_kc_glds(A, lda, m0, k0, smem[buf][0]);
      else               stage_kc_load(A, M, kend, lda, m0, k0, a_al, ra_kc);
    } else {
      stage_ko_load(A, M, kend, lda, m0, k0, a_al2, ra_ko);
    }
    if (B_KC) {
      if (b_glds && kin) stage_kc_glds(B, ldb, n0, k0, smem[buf][1]);
      else               stage_kc_load(B, N, kend, ldb, n0, k0, b_al, rb_kc);
    } else {
      stage_ko_load(B, N, kend, ldb, n0, k0, b_al2, rb_ko);
    }
  };
  auto write_tiles = [&](int buf, int k0) {
    const bool kin = k0 + BK <= kend;
    if (A_KC) {
      if (!(a_glds && kin)) stage_write_kc_natural(smem[buf][0], ra_kc);
    } else {
      stage_write_ko(smem[buf][0], ra_ko);
    }
    if (B_KC) {
      if (!(b_glds && kin)) stage_write_kc_natural(smem[buf][1], rb_kc);
    } else {
      stage_write_ko(smem[buf][1], rb_ko);
    }
  };

  load_tiles(kbeg, 0);
  write_tiles(0, kbeg);
  __syncthreads();

  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    if (t + 1 < nk)
      load_tiles(kbeg + (t + 1) * BK, cur ^ 1);  // issue early (T14)

    const bf16_t* sa = smem[cur][0];
    const bf16_t* sb = smem[cur][1];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[i] = frag(sa, wm + i * 16, lane, kk);
        bfr[i] = frag(sb, wn + i * 16, lane, kk);
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
    }

    if (t + 1 < nk) write_tiles(cur ^ 1, kbeg + (t + 1) * BK);
    __syncthreads();
  }

  // epilogue: C/D fragment mapping (16x16x32): col = lane&15,
  // row = (lane>>4)*4 + e
  float bv[4];
  if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wn + ni * 16 + (lane & 15);
      bv[ni] = (n < N) ? bf2f(bias[n]) : 0.0f;
    }
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wn + ni * 16 + (lane & 15);
      if (n >= N) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + wm + mi * 16 + (lane >> 4) * 4 + e;
        if (m >= M) continue;
        float v = acc[mi][ni][e];
        if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) v += bv[ni];
        const int64_t off = (int64_t)m * ldc + n;
        if (F32OUT) {
          Cf[off] = v;
          continue;
        }
        if (EPI >= 2) {
          // round pre-act to bf16 first (matches ops/reference.py semantics)
          const bf16_t pre = f2bf(v);
          Cpre[off] = pre;
          v = gelu_f(bf2f(pre));
        }
        C[off] = f2bf(v);
      }
    }
  }
}

// Column sums from the parts the 256 kernel's CS variant wrote (nparts
// vectors of m floats). Block `blk` owns CS_COLS columns; its CS_GROUPS
// thread groups each add every CS_GROUPS-th part in index order (up to 128
// parts per column at the flagship shapes: one thread per column would
// chain that many dependent loads), then group 0 adds the group sums in
// group order and rounds to bf16 once. All fp32, a fixed order, no
// atomics: the same bits on every call.
constexpr int CS_COLS = 32, CS_GROUPS = NTHREADS / CS_COLS;

DEV_INLINE void colsum_reduce(const float* __restrict__ parts,
                              bf16_t* __restrict__ out, int nparts, int m,
                              int blk, float* sh) {
  const int c = threadIdx.x % CS_COLS, g = threadIdx.x / CS_COLS;
  const int i = blk * CS_COLS + c;
  float acc = 0.f;
  if (i < m) {
#pragma unroll 4
    for (int p = g; p < nparts; p += CS_GROUPS)
      acc += parts[(int64_t)p * m + i];
  }
  sh[g * CS_COLS + c] = acc;
  __syncthreads();
  if (g == 0 && i < m) {
    float s = sh[c];
#pragma unroll
    for (int q = 1; q < CS_GROUPS; ++q) s += sh[q * CS_COLS + c];
    out[i] = f2bf(s);
  }
}

__global__ void colsum_reduce_kernel(const float* __restrict__ parts,
                                     bf16_t* __restrict__ out, int nparts,
                                     int m) {
  __shared__ float sh[NTHREADS];
  colsum_reduce(parts, out, nparts, m, blockIdx.x, sh);
}

// The first cs_blocks blocks (0 without cs_out) reduce the column-sum parts
// in the same launch, ahead of the blocks that reduce the product partials
// so they are not its tail.
__global__ void splitk_reduce_kernel(const float* __restrict__ parts,
                                     bf16_t* __restrict__ out, int nparts,
                                     int64_t mn, int cs_blocks,
                                     const float* __restrict__ cs_parts,
                                     bf16_t* __restrict__ cs_out,
                                     int cs_nparts, int cs_m) {
  __shared__ float sh[NTHREADS];
  if ((int)blockIdx.x < cs_blocks) {  // block-uniform
    colsum_reduce(cs_parts, cs_out, cs_nparts, cs_m, blockIdx.x, sh);
    return;
  }
  const int blk = blockIdx.x - cs_blocks;
  const int64_t stride = (int64_t)(gridDim.x - cs_blocks) * blockDim.x * 4;
  for (int64_t i = ((int64_t)blk * blockDim.x + threadIdx.x) * 4;
       i < mn; i += stride) {
    if (i + 4 <= mn) {
      f32x4 sv = *reinterpret_cast<const f32x4*>(parts + i);
      for (int p = 1; p < nparts; ++p) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(parts + p * mn + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[e] += v[e];
      }
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(sv[e]);
      *reinterpret_cast<bf16x4*>(out + i) = o;
    } else {
      for (int64_t j = i; j < mn; ++j) {
        float acc = 0.f;
        for (int p = 0; p < nparts; ++p) acc += parts[p * mn + j];
        out[j] = f2bf(acc);
      }
    }
  }
}

void splitk_reduce(const float* parts, bf16_t* out, int nparts, int64_t mn,
                   const float* cs_parts, bf16_t* cs_out, int cs_nparts,
                   int cs_m, hipStream_t stream) {
  const int blocks = std::max(1, (int)std::min<int64_t>(
      (mn / 4 + NTHREADS - 1) / NTHREADS, 2048));
  const int cs_blocks = cs_out ? (cs_m + CS_COLS - 1) / CS_COLS : 0;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(cs_blocks + blocks),
                     dim3(NTHREADS), 0, stream, parts, out, nparts, mn,
                     cs_blocks, cs_parts, cs_out, cs_nparts, cs_m);
}

}  // namespace

void gemm_bf16(const void* A, const void* B, void* C, void* c_pre,
               const void* bias, int M, int N, int K, int lda, int ldb,
               int ldc, int64_t stride_a, int64_t stride_b, int64_t stride_c,
               int batch, bool a_kc, bool b_kc, int epi, float* splitk_ws,
               void* colsum_out, hipStream_t stream) {
  const GemmPlan p = gemm_plan(M, N, K, lda, ldb, a_kc, b_kc, epi, batch);
  if (p.kernel == 0)
    throw std::runtime_error(std::string("gemm_bf16: ") + p.why_not);
  const bool colsum = colsum_out != nullptr;
  if (colsum) {
    if (const char* why = colsum_why_not(p, a_kc, b_kc, batch))
      throw std::runtime_error(std::string("gemm_bf16: ") + why);
    if (splitk_ws == nullptr)
      throw std::runtime_error(
          "gemm_bf16: colsum_out needs a workspace of " +
          std::to_string(gemm_ws_floats(p, M, N, true)) + " floats");
  }

  // split-K: chunk z writes fp32 partials [M, N] at splitk_ws + z*M*N,
  // reduced into C (contiguous) by a second launch
  const bool split = p.split_k > 1;
  const int64_t mn = (int64_t)M * N;
  if (split && splitk_ws == nullptr)
    throw std::runtime_error("gemm_bf16: split-K plan needs a workspace of " +
                             std::to_string(gemm_ws_floats(p, M, N, false)) +
                             " floats");
  if (split && ldc != N)
    throw std::runtime_error("gemm_bf16: split-K plan needs ldc == N");
  void* out = C;
  if (split) {
    out = splitk_ws;
    stride_c = mn;
  }
  // column-sum parts follow the product partials in the workspace
  float* cs_parts =
      colsum ? splitk_ws + gemm_ws_floats(p, M, N, false) : nullptr;
  const int cs_nparts = p.split_k * (N / plan::T256);

  if (p.kernel == plan::T256) {
    gemm256_bf16(A, B, out, c_pre, bias, M, N, K, lda, ldb, ldc, stride_a,
                 stride_b, stride_c, batch, /*k_outer=*/!a_kc, epi, p.split_k,
                 p.k_chunk, cs_parts, stream);
  } else {
    const int nbx = (N + BN - 1) / BN, nby = (M + BM - 1) / BM;
    const dim3 grid(nbx * nby, 1, split ? p.split_k : batch), block(NTHREADS);
    const bf16_t* a = static_cast<const bf16_t*>(A);
    const bf16_t* b = static_cast<const bf16_t*>(B);
    bf16_t* cp = static_cast<bf16_t*>(c_pre);
    const bf16_t* bi = static_cast<const bf16_t*>(bias);
#define GEMM_LAUNCH(AKC, BKC, E, F32)                                       \
    hipLaunchKernelGGL((gemm_kernel<AKC, BKC, E, F32>), grid, block, 0,     \
                       stream, a, b, out, cp, bi, M, N, K, lda, ldb, ldc,   \
                       stride_a, stride_b, stride_c, p.k_chunk)
#define GEMM_EPI(AKC, BKC)                                                  \
    if (split) { GEMM_LAUNCH(AKC, BKC, 0, true); }                          \
    else switch (epi) {  /* the plan admits epi 0..3 here */                \
      case EPI_NONE: GEMM_LAUNCH(AKC, BKC, EPI_NONE, false); break;         \
      case EPI_BIAS: GEMM_LAUNCH(AKC, BKC, EPI_BIAS, false); break;         \
      case EPI_BIAS_GELU: GEMM_LAUNCH(AKC, BKC, EPI_BIAS_GELU, false); break; \
      case EPI_GELU: GEMM_LAUNCH(AKC, BKC, EPI_GELU, false); break;         \
    }
    if (a_kc && b_kc) { GEMM_EPI(true, true); }
    else if (a_kc && !b_kc) { GEMM_EPI(true, false); }
    else if (!a_kc && b_kc) { GEMM_EPI(false, true); }
    else { GEMM_EPI(false, false); }
#undef GEMM_EPI
#undef GEMM_LAUNCH
  }
  if (split) {
    HIP_CHECK(hipGetLastError());
    splitk_reduce(splitk_ws, static_cast<bf16_t*>(C), p.split_k, mn,
                  cs_parts, static_cast<bf16_t*>(colsum_out), cs_nparts, M,
                  stream);
  } else if (colsum) {
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(colsum_reduce_kernel,
                       dim3((M + CS_COLS - 1) / CS_COLS), dim3(NTHREADS), 0,
                       stream, cs_parts, static_cast<bf16_t*>(colsum_out),
                       cs_nparts, M);
  }
}

}  // namespace tepdist
