// Deep-pipelined 256x256 bf16 GEMM for gfx950 (the guide's 8-phase
// counted-vmcnt template, re-derived for this kernel set).
//
// Geometry: 256x256 tile, BK=64, 8 waves (2M x 4N), per-wave output
// 128(M) x 4x16(N, STRIDED: wave wn owns n = p*64 + wn*16 for phase
// p=0..3). K-loop phase p computes all 8 m-fragments against the phase's
// n-fragment (16 MFMAs); A fragments (16 x bf16x8) load once per K-tile at
// phase 0 and live in registers.
//
// Staging: global_load_lds only, in 8 KiB QUARTER units (64 rows x 64 cols,
// one dwordx4 per thread), 8 units per K-tile, two staged per phase, slots
// cycling mod 8 per operand (2 tiles of LDS per operand = 128 KiB total).
// The schedule guarantees each unit's slot had its last reader one raw
// barrier earlier: A(t) quarters are consumed entirely at t.ph0 (register
// A), B(t,q_p) at t.ph_p; stages run A(t+2,q01)@t.ph1, A(t+2,q23)@t.ph2,
// B(t+2,q01)@t.ph3, B(t+2,q23)@(t+1).ph0. All barriers are RAW s_barrier
// (no vmcnt drain: __syncthreads would wait the in-flight DMAs to 0) and a
// single counted s_waitcnt vmcnt(6) per K-tile keeps 6 quarter-units (3
// "half-tiles") in flight.
//
// Stagger. Waves w and w+4 share a SIMD and differ in wm, so in lockstep
// both read LDS together and issue MFMAs together. Waves 4..7 (the "late"
// half, wm == 1) therefore take one extra barrier in front of the K loop
// and waves 0..3 (the "early" half) one behind it: on every SIMD one wave is
// in its MFMA cluster while its partner reads fragments and stages. Number
// the phases j = 4t + p, call phase j's read+stage segment R_j and its MFMA
// segment M_j, and count barrier instances so that the early half runs R_j
// between instances 2j-1 and 2j and M_j between 2j and 2j+1; the late half
// runs both one instance later. Every wave stages a share of every unit, and
// a wave's counted wait covers its own DMAs only. Two rules follow:
//  RAW  a wait in R_w is passed by the late half before instance 2w+1, which
//       the early half passes before R_{w+1}: waits sit in R segments (in
//       front of the phase's first barrier) and the first read of what they
//       retire is one phase later. A wait in M_w would be too late.
//  WAR  reads issued in R_r retire at the lgkmcnt(0) that heads M_r. For
//       early readers that is before instance 2r+1, and the earliest
//       restage, the early half's R_{r+1}, comes after it. For late readers
//       it is before 2r+2 only, so their slot may be restaged in R_{r+2}, or
//       in R_{r+1} if the lgkmcnt(0) stands in front of R_r's barrier.
// Every staged unit of tile t, j0 = 4t (steady state):
//   unit      staged    retired by     read     readers  restaged
//   A(t,q01)  R_{j0-7}  wait R_{j0-1}  R_{j0}   early    R_{j0+1}  r+1, early
//   A(t,q23)  R_{j0-6}  wait R_{j0-1}  R_{j0}   late     R_{j0+2}  r+2
//   B(t,q0)   R_{j0-5}  wait R_{j0-1}  R_{j0}   both     R_{j0+3}  r+3
//   B(t,q1)   R_{j0-5}  wait R_{j0-1}  R_{j0+1} both     R_{j0+3}  r+2
//   B(t,q2)   R_{j0-4}  wait R_{j0-1}  R_{j0+2} both     R_{j0+4}  r+2
//   B(t,q3)   R_{j0-4}  wait R_{j0-1}  R_{j0+3} both     R_{j0+4}  r+1 (*)
// (*) phase 3 waits lgkmcnt(0) in front of its first barrier, both layouts.
// Each unit is read in one phase only. The wait of R_{j0-1}, phase 3 of tile
// t-1, is vmcnt(6) behind stage_b(t+1, 0): A(t+1) and B(t+1,q01) stay in
// flight, all of tile t is retired.
//  Prologue: tile 0 and A(1), B(1,q01) are staged, vmcnt(6) retires tile 0
//   in front of the barrier every wave takes before R_0; no slot is reused.
//   A(1), B(1,q01) and B(1,q23) (staged in R_0) retire at the wait of R_3.
//  nk == 2: nothing is staged after R_0 and R_3 waits vmcnt(0).
//  nk == 3: R_1..R_3 stage A(2), B(2,q01), vmcnt(6) retires tile 1; R_4
//   restages B(0,q23) as B(2,q23) by (*); R_7 waits vmcnt(0).
//  Last tile: tile nk-2 stages nothing in phases 1..3, so no count would
//   push B(nk-1,q23) out; its phase 3 waits vmcnt(0), one phase before the
//   first read of tile nk-1. (A vmcnt(0) + barrier in front of the last
//   tile would let the early half read past a wait the late half has not
//   reached.)
//  Epilogue: after the early half's extra barrier every wave waits
//   lgkmcnt(0) and takes one more; no DMA is in flight and every fragment
//   read has retired when the output image overwrites the slots.
// Each wave issues 16 MFMAs per phase; the 4 column-sum MFMAs fall to every
// wave of a block in the same phase 0, so the halves stay equal.
//
// Two operand layouts, both with M,N % 256 == 0, K % 64 == 0, 16B-aligned
// rows and >= 2 K-tiles per chunk (gemm_plan.h decides when that holds,
// gemm.hip covers the rest):
//  - canonical: both operands k-contiguous (A [M][K], B [N][K]);
//  - k-outer (KO = true): both operands stored [K][F] (A [K][M], B [K][N]),
//    wgrad's dy and x as they lie in memory. A quarter unit is then the
//    natural [64 k][64 f] image, staged by the same stage_q with the row
//    and column roles swapped, and the fragments are read with the map of
//    tr_frag<BK> (lds_frag.h; two ds_read_b64_tr_b16 each, conflict-free
//    at 64-column rows). That map permutes k within each 32-block; both
//    operands go through it, so the products pair up unchanged. Schedule,
//    slots, barriers, split-K and epilogues are the canonical ones.
// Mixed layouts (dgrad's weight) are not handled: linear_bwd transposes the
// weight, a few microseconds.

#include <stdexcept>

#include "common.h"
#include "gemm_tile.h"
#include "kernels.h"

namespace tepdist {

namespace {

constexpr int BM = plan::T256, BN = plan::T256, BK = plan::BK;
constexpr int NTH = 512;  // 8 waves
constexpr int QROWS = 64;          // stage-unit rows
constexpr int SLOT_E = QROWS * BK; // elements per slot (8 KiB)

// swizzled offset within a [64][64] slot / the [256][64] epilogue image
DEV_INLINE int qoff(int row, int col_e) { return loff<BK>(row, col_e); }

// stage one quarter unit: rows [f0, f0+64) x cols [k0, k0+64) of a
// k-contiguous operand into slot `dst` (one glds dwordx4 per thread). A
// k-outer operand passes (k0, f0) instead: rows are k, columns features.
DEV_INLINE void stage_q(const bf16_t* __restrict__ src, int64_t ld, int f0,
                        int k0, bf16_t* dst) {
  const int wave = threadIdx.x >> 6;
  const int row = threadIdx.x >> 3;          // 0..63 (lane-linear per wave)
  const int c = (threadIdx.x & 7) * 8;
  const int ksrc = k0 + (c ^ (SWZ8(row) << 3));  // inverse swizzle on source
  const bf16_t* g = src + (int64_t)(f0 + row) * ld + ksrc;
  bf16_t* l = dst + (8 * wave) * BK;         // wave-uniform base
  __builtin_amdgcn_global_load_lds((glds_src_t)g, (glds_dst_t)l, 16, 0, 0);
}

// f32 image variant of the swizzle (16B slot = 4 floats)
DEV_INLINE int qoff_f32(int row, int col_e) {
  return row * BK + (col_e ^ (SWZ8(row) << 2));
}

DEV_INLINE bf16x8 fragq(const bf16_t* slot, int row, int col_e) {
  return *reinterpret_cast<const bf16x8*>(slot + qoff(row, col_e));
}

// tr_frag<BK> (lds_frag.h: same lanes, same addresses, same k order) with
// its two ds_read_b64_tr_b16 written as inline asm. Through the builtin the
// compiler takes the read for an ordinary load beside the in-flight
// global_load_lds DMAs and puts s_waitcnt vmcnt(0) in front of every group
// of reads, which drains the counted-vmcnt(6) pipeline four times per
// K-tile. The compiler does not count these reads, so the caller waits
// lgkmcnt(0) itself before the first use (LGKM_WAIT_KO below). The k half
// KK and the +16-row second read are immediate offsets: the swizzle only
// looks at row bits 1..3.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const bf16_t* lds_cptr_t;

template <int OFF>
DEV_INLINE bf16x4 tr_read_asm(uint32_t addr) {
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(v)
               : "v"(addr), "n"(OFF)
               : "memory");
  return __builtin_bit_cast(bf16x4, v);
}

template <int KK>
DEV_INLINE bf16x8 tr_frag_asm(const bf16_t* slot, int df, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const uint32_t addr = (uint32_t)(uintptr_t)(lds_cptr_t)(
      slot + qoff(4 * g + (i >> 2), 16 * df + 4 * (i & 3)));
  const bf16x4 lo = tr_read_asm<KK * 32 * BK * 2>(addr);
  const bf16x4 hi = tr_read_asm<(KK * 32 + 16) * BK * 2>(addr);
  bf16x8 f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = lo[e];
    f[e + 4] = hi[e];
  }
  return f;
}

// MFMA fragment of 16 features x 32 k from one slot: feature block df
// (0..3), k half KK (0..1). Canonical slots are [f][k] images, k-outer ones
// [k][f] read transposed. Wave-uniform call sites only (the transposed read
// gathers across all 64 lanes).
template <bool KO, int KK>
DEV_INLINE bf16x8 frag_fk(const bf16_t* slot, int df, int lane) {
  if (KO) return tr_frag_asm<KK>(slot, df, lane);
  return fragq(slot, df * 16 + (lane & 15), 8 * (lane >> 4) + 32 * KK);
}

#define RAW_BAR() __builtin_amdgcn_s_barrier()
#define VMCNT6() asm volatile("s_waitcnt vmcnt(6)" ::: "memory")
// k-outer fragments come from inline-asm reads: wait for them by hand, and
// keep the scheduler from lifting the register-only MFMAs over the wait.
#define LGKM_WAIT_KO()                                      \
  do {                                                      \
    if (KO) {                                               \
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    \
      __builtin_amdgcn_sched_barrier(0);                    \
    }                                                       \
  } while (0)

// CS (k-outer, plain epilogue only): the block also sums A over the rows k
// of its K-tiles, colsum[m] = sum_k A[k][m] (wgrad's bias gradient), from
// the A fragments phase 0 already holds: one MFMA per fragment against a
// ones B fragment, every column of the result the same sum. The N/256
// blocks that share an A panel take its K-tiles in turn (block j the tiles
// t of its chunk with t % nbx == j) and within a block wave (wm, wn) takes
// m-fragments 2wn, 2wn+1 of its half, so each element is summed once. Each
// block stores its fp32 part, zeros included, at colsum + (z*nbx + j)*M:
// nothing to zero-fill, no atomics; the reduce kernels of gemm.hip add the
// parts in fixed order.
template <int EPI, bool F32OUT = false, bool KO = false, bool CS = false>
__launch_bounds__(NTH, 1) __global__
void gemm256_kernel(const bf16_t* __restrict__ A,
                    const bf16_t* __restrict__ B, void* __restrict__ Cv,
                    bf16_t* __restrict__ Cpre,
                    const bf16_t* __restrict__ bias, int M, int N, int K,
                    int lda, int ldb, int ldc, int64_t strideA,
                    int64_t strideB, int64_t strideC, int k_chunk,
                    float* __restrict__ colsum) {
  static_assert(!CS || (KO && EPI == EPI_NONE), "CS: k-outer, plain epilogue");
  bf16_t* C = static_cast<bf16_t*>(Cv);
  float* Cf = static_cast<float*>(Cv);
  int kbeg = 0, kend = K;
  if (F32OUT) {  // split-K: blockIdx.z = K-chunk, fp32 partial output
    kbeg = blockIdx.z * k_chunk;
    kend = min(K, kbeg + k_chunk);
    Cf += blockIdx.z * strideC;
    if (kend <= kbeg) kbeg = kend = 0;  // dead chunk: no loads, zero out
  } else {
    A += blockIdx.z * strideA;
    B += blockIdx.z * strideB;
    C += blockIdx.z * strideC;
    if (EPI >= 2) Cpre += blockIdx.z * strideC;
  }

  const int nbx = N / BN;
  const int swz = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (swz / nbx) * BM, n0 = (swz % nbx) * BN;

  __shared__ bf16_t smem[16 * SLOT_E];  // A slots 0..7, B slots 8..15
  bf16_t* const aslot = smem;
  bf16_t* const bslot = smem + 8 * SLOT_E;

  const int lane = threadIdx.x & 63;
  const int wm = (threadIdx.x >> 8) & 1;       // wave row (0..1)
  const int wn = (threadIdx.x >> 6) & 3;       // wave col (0..3)

  f32x4 acc[8][4] = {};

  const int nk = (kend - kbeg) / BK;

  // A quarter q of tile t covers features m0 + 64q; B quarter: n0 + 64q.
  auto stage_1 = [&](const bf16_t* __restrict__ src, int ld, int f0, int t,
                     bf16_t* dst) {
    if (KO) stage_q(src, ld, kbeg + t * BK, f0, dst);
    else    stage_q(src, ld, f0, kbeg + t * BK, dst);
  };
  auto stage_a = [&](int t, int q2) {  // stage quarters q2 and q2+1
    stage_1(A, lda, m0 + 64 * q2, t, aslot + ((4 * t + q2) & 7) * SLOT_E);
    stage_1(A, lda, m0 + 64 * (q2 + 1), t,
            aslot + ((4 * t + q2 + 1) & 7) * SLOT_E);
  };
  auto stage_b = [&](int t, int q2) {
    stage_1(B, ldb, n0 + 64 * q2, t, bslot + ((4 * t + q2) & 7) * SLOT_E);
    stage_1(B, ldb, n0 + 64 * (q2 + 1), t,
            bslot + ((4 * t + q2 + 1) & 7) * SLOT_E);
  };

  // prologue: tile 0 fully + tile 1's A and B q0,q1 (14 units in flight),
  // then complete tile 0 (vmcnt 6) before its reads.
  if (nk > 0) {
    stage_a(0, 0);
    stage_a(0, 2);
    stage_b(0, 0);
    stage_b(0, 2);
    if (nk > 1) {
      stage_a(1, 0);
      stage_a(1, 2);
      stage_b(1, 0);
    }
    VMCNT6();
  }
  RAW_BAR();
  // the stagger (header): waves 4..7 start one barrier late, waves 0..3
  // make it up after the loop
  const bool late = __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256;
  if (late) RAW_BAR();

  // CS: this block's turn comes every nbx-th K-tile, starting at its n-tile
  // index; wave-uniform scalars, so the extra MFMAs sit behind scalar tests
  const int cs_wn = CS ? __builtin_amdgcn_readfirstlane(wn) : 0;
  int cs_next = swz % nbx;
  f32x4 cs[2] = {};
  bf16x8 ones;
  if (CS) {
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = f2bf(1.0f);
  }

  bf16x8 af[8][2];
  for (int t = 0; t < nk; ++t) {
    // ---- phase 0: read ALL A fragments + B fragment 0; stage B(t+1,q23)
    {
      const bf16_t* as0 = aslot + ((4 * t + 2 * wm) & 7) * SLOT_E;
      const bf16_t* as1 = aslot + ((4 * t + 2 * wm + 1) & 7) * SLOT_E;
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) {
        const bf16_t* s = (mi < 4) ? as0 : as1;
        af[mi][0] = frag_fk<KO, 0>(s, mi & 3, lane);
        af[mi][1] = frag_fk<KO, 1>(s, mi & 3, lane);
      }
      bf16x8 bf0[2];
      {
        const bf16_t* bs = bslot + ((4 * t + 0) & 7) * SLOT_E;
        bf0[0] = frag_fk<KO, 0>(bs, wn, lane);
        bf0[1] = frag_fk<KO, 1>(bs, wn, lane);
      }
      if (t + 1 < nk) stage_b(t + 1, 2);
      RAW_BAR();
      LGKM_WAIT_KO();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          acc[mi][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi][kk], bf0[kk], acc[mi][0], 0, 0, 0);
      if (CS && t == cs_next) {
        cs_next += nbx;
#pragma unroll
        for (int w = 0; w < 4; ++w)  // af is indexed statically: 4 cases
          if (w == cs_wn) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
              for (int h = 0; h < 2; ++h)
                cs[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    af[2 * w + h][kk], ones, cs[h], 0, 0, 0);
          }
      }
      __builtin_amdgcn_s_setprio(0);
      RAW_BAR();
    }
    // ---- phases 1..3: read B fragment p; stage per schedule
#pragma unroll
    for (int p = 1; p < 4; ++p) {
      bf16x8 bfp[2];
      {
        const bf16_t* bs = bslot + ((4 * t + p) & 7) * SLOT_E;
        bfp[0] = frag_fk<KO, 0>(bs, wn, lane);
        bfp[1] = frag_fk<KO, 1>(bs, wn, lane);
      }
      if (p == 1 && t + 2 < nk) stage_a(t + 2, 0);
      if (p == 2 && t + 2 < nk) stage_a(t + 2, 2);
      if (p == 3) {
        // tile boundary, in front of the phase's first barrier (RAW rule of
        // the header): past vmcnt(6) only A(t+2) and B(t+2,q01) are in
        // flight, tile t+1 is whole. Tile nk-2 has nothing to stage and
        // drains B(nk-1,q23), which no later stage would push past a count.
        if (t + 2 < nk) {
          stage_b(t + 2, 0);
          VMCNT6();
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        // WAR rule: B(t,q3) is restaged one phase on, so these reads retire
        // before the barrier, in both layouts
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
      RAW_BAR();
      if (p != 3) LGKM_WAIT_KO();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          acc[mi][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi][kk], bfp[kk], acc[mi][p], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      RAW_BAR();
    }
  }
  if (!late) RAW_BAR();  // waves 0..3 wait out the late half's last cluster

  // ---- column sums: all 16 result columns are equal, the lanes of column
  // 0 store rows 4*(lane>>4) + e of m-fragments 2wn, 2wn+1
  if (CS) {
    float* part = colsum +
        ((int64_t)(F32OUT ? blockIdx.z : 0) * nbx + swz % nbx) * M + m0 +
        wm * 128 + wn * 32 + 4 * (lane >> 4);
    if ((lane & 15) == 0) {
      *reinterpret_cast<f32x4*>(part) = cs[0];
      *reinterpret_cast<f32x4*>(part + 16) = cs[1];
    }
  }

  // ---- epilogue (phase-p fragment n-columns: n = 64p + wn*16) ----
  float bv[4];
  if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      bv[p] = bf2f(bias[n0 + 64 * p + wn * 16 + (lane & 15)]);
  }
  if (!F32OUT) {
    // Bounce the output through LDS so global stores are whole 128-byte
    // cachelines: the C-fragment layout is column-strided (per lane, the
    // four accumulator elements are CONSECUTIVE ROWS of one column), so a
    // direct scatter is 2-byte stores in 32-byte segments — at K ~ 1k the
    // C write-out dominates per-block overhead. One 64-column phase at a
    // time: waves deposit fragments into a swizzled [256][64] image, then
    // all 512 threads store it row-major (8 lanes = one full row).
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // gelu epilogues stage only the PRE-activation image; gelu is applied
    // at store time on the vector chunks (halves the LDS traffic of the
    // dual-output fc epilogue)
    bf16_t* img = smem;                  // [256][64]
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int cl = wn * 16 + (lane & 15);
#pragma unroll
      for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = wm * 128 + mi * 16 + (lane >> 4) * 4 + e;
          float v = acc[mi][p][e];
          if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) v += bv[p];
          img[qoff(row, cl)] = f2bf(v);
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const int sr = threadIdx.x >> 3;         // 64 rows per round
      const int c8 = (threadIdx.x & 7) * 8;    // 16B chunk within the row
#pragma unroll
      for (int rr = 0; rr < BM; rr += 64) {
        const int row = rr + sr;
        const int64_t off = (int64_t)(m0 + row) * ldc + n0 + 64 * p + c8;
        bf16x8 v8 = *reinterpret_cast<const bf16x8*>(img + qoff(row, c8));
        if (EPI == EPI_DGELU) {
          const bf16x8 pv = *reinterpret_cast<const bf16x8*>(Cpre + off);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            v8[e] = f2bf(bf2f(v8[e]) * gelu_grad_f(bf2f(pv[e])));
        } else if (EPI >= 2) {
          *reinterpret_cast<bf16x8*>(Cpre + off) = v8;
#pragma unroll
          for (int e = 0; e < 8; ++e) v8[e] = f2bf(gelu_f(bf2f(v8[e])));
        }
        *reinterpret_cast<bf16x8*>(C + off) = v8;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // image free for the next phase
    }
    return;
  }
  // F32OUT (split-K partials): same LDS bounce with a [256][64] f32 image
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  {
    float* imgf = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int cl = wn * 16 + (lane & 15);
#pragma unroll
      for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = wm * 128 + mi * 16 + (lane >> 4) * 4 + e;
          imgf[qoff_f32(row, cl)] = acc[mi][p][e];
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const int sr = threadIdx.x >> 4;         // 32 rows per round
      const int c4 = (threadIdx.x & 15) * 4;   // 16B chunk (4 floats)
#pragma unroll
      for (int rr = 0; rr < BM; rr += 32) {
        const int row = rr + sr;
        const int64_t off = (int64_t)(m0 + row) * ldc + n0 + 64 * p + c4;
        *reinterpret_cast<f32x4*>(Cf + off) =
            *reinterpret_cast<const f32x4*>(imgf + qoff_f32(row, c4));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }
}

}  // namespace

// Launches what gemm_plan() planned for the 256 kernel: split_k > 1 writes
// fp32 partials (C is then the workspace), chunk z at C + z*stride_c.
// k_outer: both operands stored [K][F] (plain epilogue only). colsum_parts
// (k_outer and batch 1 only, else null): split_k * (N/256) vectors of M
// floats, all written, whose sum over the parts is A's column sums.
void gemm256_bf16(const void* A, const void* B, void* C, void* c_pre,
                  const void* bias, int M, int N, int K, int lda, int ldb,
                  int ldc, int64_t stride_a, int64_t stride_b,
                  int64_t stride_c, int batch, bool k_outer, int epi,
                  int split_k, int k_chunk, float* colsum_parts,
                  hipStream_t stream) {
  const bool split = split_k > 1;
  const dim3 grid((N / BN) * (M / BM), 1, split ? split_k : batch), block(NTH);
  const bf16_t* a = static_cast<const bf16_t*>(A);
  const bf16_t* b = static_cast<const bf16_t*>(B);
  bf16_t* cp = static_cast<bf16_t*>(c_pre);
  const bf16_t* bi = static_cast<const bf16_t*>(bias);
#define G256(E, F32, KO, CS)                                               \
  hipLaunchKernelGGL((gemm256_kernel<E, F32, KO, CS>), grid, block, 0,     \
                     stream, a, b, C, cp, bi, M, N, K, lda, ldb, ldc,      \
                     stride_a, stride_b, stride_c, k_chunk, colsum_parts)
  if (k_outer) {
    if (epi != EPI_NONE)
      throw std::runtime_error(
          "gemm256_bf16: k-outer operands have only the plain epilogue");
    if (colsum_parts && batch != 1)
      throw std::runtime_error("gemm256_bf16: column sums need batch 1");
    if (colsum_parts) {
      if (split) { G256(EPI_NONE, true, true, true); }
      else { G256(EPI_NONE, false, true, true); }
    }
    else if (split) { G256(EPI_NONE, true, true, false); }
    else { G256(EPI_NONE, false, true, false); }
  } else if (colsum_parts) {
    throw std::runtime_error(
        "gemm256_bf16: column sums need two k-outer operands");
  } else if (split) { G256(EPI_NONE, true, false, false); }
  else switch (epi) {
    case EPI_NONE: G256(EPI_NONE, false, false, false); break;
    case EPI_BIAS: G256(EPI_BIAS, false, false, false); break;
    case EPI_BIAS_GELU: G256(EPI_BIAS_GELU, false, false, false); break;
    case EPI_GELU: G256(EPI_GELU, false, false, false); break;
    case EPI_DGELU: G256(EPI_DGELU, false, false, false); break;
  }
#undef G256
}

}  // namespace tepdist
