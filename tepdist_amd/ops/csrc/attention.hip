// Fused flash-style causal attention (forward + backward) for gfx950.
// Replaces the composed scores-GEMM + softmax + PV path (SURVEY.md §2.9:
// the reference leaves attention to XLA codegen); docs/KERNELS.md has the
// full design discussion.
//
// Forward: one block = 512 q rows (D=128: 256), 8 waves sharing the
// double-buffered K/V staging; at D=64 wave w owns the 32-row pairs w and
// 15-w so the causal mask leaves every wave the same work. Scores are
// computed TRANSPOSED (S^T = mfma(K, Q)) so softmax state is per-lane (two
// shfl_xor per reduction) and P^T feeds the PV MFMA straight from the
// accumulators via the k-permutation invariance; O accumulates as O^T and
// scatters once. Saves per-row logsumexp; the S x S score matrix never
// touches HBM.
//
// Backward: TWO atomics-free kernels (the classic fused flash2 backward
// spends most of its time on dQ atomicAdd traffic — measured with the
// section probe, see profiles/):
//   - dK/dV kernel: block = 256 kv rows (D=128: 128) as 128-row slabs, 8
//     waves x 16-kv slices sharing the Q/dO tile staging; S = mfma(Q, K)
//     untransposed puts kv in the lane index so dV^T/dK^T consume P/dS from
//     the accumulators (k-permuted). Slices wholly above the causal
//     diagonal of a q tile are skipped.
//   - dQ kernel: forward-shaped (same pair ownership), dQ^T accumulated in
//     registers, bf16 output written directly in the packed-qkv strided
//     layout.
// delta = rowsum(dO*O) is the flash2 preprocess.
//
// Every streamed tile (K, V, Q, dO) is fetched once with 16B row loads and
// kept as ONE natural [rows][D] LDS image. The products that need it
// transposed (V^T in fwd, dO^T/Q^T in dK/dV, K^T in dQ) form their
// A-fragments at read time with ds_read_b64_tr_b16 (tr_frag, lds_frag.h).
// Row constants are folded: every P is exp2 of one fma with scale*log2e
// (fwd: -m*log2e per lane; backward: -lse*log2e), dS is formed without
// `scale`, and `scale` is applied once to the dK/dQ accumulators at the
// store.

#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "lds_frag.h"

namespace tepdist {

namespace {

constexpr int NT = 256;
constexpr int QB = 128;   // q rows per block (fwd)
constexpr int KB = 64;    // kv rows per tile

// branchless exp: one v_exp_f32, no libcall special-casing. Arguments are
// always <= 0 here (running-max subtraction / masked to -3e38), so the only
// edge is underflow to 0 — exactly what the hardware instruction does.
constexpr float kLog2e = 1.4426950408889634f;
DEV_INLINE float fast_exp(float x) {
  return __builtin_amdgcn_exp2f(x * kLog2e);
}

// execution barrier with LDS-visibility only: s_waitcnt lgkmcnt(0) then a
// raw s_barrier. Unlike __syncthreads there is NO vmcnt(0) drain, so
// in-flight global prefetch loads and the fire-and-forget dQ atomics keep
// flowing across tile boundaries instead of serializing at each barrier.
#define BAR_LDS()                                        \
  do {                                                   \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
    __builtin_amdgcn_s_barrier();                        \
  } while (0)

DEV_INLINE float warp16_max(float v) {
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

DEV_INLINE float warp16_sum(float v) {
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

// Forward layout (CDNA-native): compute S^T = mfma(K, Q) so the score
// C-fragment holds q in the lane index (q = lane&15) and kv across lane
// groups/elements. Softmax row stats then reduce with TWO shfl_xor steps
// (strides 16, 32) and the running max/sum/alpha are pure per-lane state.
// P^T is consumed directly from the accumulators as the PV B-fragment via
// the MFMA k-permutation invariance (a consistent reorder of the k slots of
// both operands leaves the dot product unchanged): B slot (g, e) holds
// kv = 32c + 4g + e (e<4, from C-frag 2c) or 32c + 16 + 4g + (e-4) (from
// C-frag 2c+1), and the A operand (V^T, from the natural [KB][D] image) is read with
// the same kv order by two transposed 8B reads. O accumulates transposed ([d][q],
// q = lane&15 — the same lane as the softmax state, so the alpha rescale is
// a per-lane multiply) and is scattered once at the end. No P tile ever
// touches LDS.
constexpr int NTF = 512;   // 8 waves x 64 q columns (QBF = 512): the
                           // K/V staging volume per block is fixed by S,
                           // so doubling the q rows it feeds halves the
                           // staging cost per unit of MFMA work (same
                           // lever as the backward's 256-kv blocks); the
                           // 64 q are processed as two sequential 16-q
                           // pairs so the score accumulators stay [4][2]
constexpr int QBF = 512;   // D=64; D=128 uses 256 (register budget)

// First q row of the hp-th 32-row pair of a wave (fwd and dQ kernels).
// NQ=4 (D=64): the block's 16 pairs are dealt so that wave w owns pairs w
// and 15-w — under the causal mask pair p has work in ceil((32p+32)/64) kv
// tiles, so every wave gets the same total and no SIMD idles at the per-tile
// barrier while wave 7 finishes. NQ=2 (D=128): one pair per wave, in order.
template <int NQ>
DEV_INLINE int pair_row0(int q0, int wave, int hp) {
  return NQ == 4 ? q0 + 32 * (hp ? 15 - wave : wave) : q0 + 32 * wave;
}

template <int D, int NQ = (D == 64 ? 4 : 2)>  // 16-q groups per wave
__launch_bounds__(NTF) __global__
void flash_fwd_kernel(const bf16_t* __restrict__ Q,
                      const bf16_t* __restrict__ K,
                      const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
                      float* __restrict__ LSE, int S, int H, float scale,
                      bool causal, int64_t q_bs, int64_t q_hs, int64_t q_rs,
                      int64_t o_bs, int64_t o_hs, int64_t o_rs) {
  constexpr int DK = D / 32;   // k-chunks per d-contraction fragment
  constexpr int DF = D / 16;   // d row fragments of O^T
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int q0 = blockIdx.x * (128 * NQ);   // 8 waves x 16*NQ q rows
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;

  const bf16_t* qp = Q + (int64_t)b * q_bs + (int64_t)h * q_hs;
  const bf16_t* kp = K + (int64_t)b * q_bs + (int64_t)h * q_hs;
  const bf16_t* vp = V + (int64_t)b * q_bs + (int64_t)h * q_hs;
  bf16_t* op = O + (int64_t)b * o_bs + (int64_t)h * o_hs;

  // double-buffered tiles: compute reads parity (t&1) while the staging
  // writes parity ^1 — one barrier per tile instead of two
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * 2 * KB * D];
  const int BUFSZ = 2 * KB * D;   // K and V, both natural [KB][D]

  // Q fragments (PV B-layout twin): nf-th 16-q group, kk-th 32-d chunk
  bf16x8 qf[NQ][DK];
#pragma unroll
  for (int nf = 0; nf < NQ; ++nf)
#pragma unroll
    for (int kk = 0; kk < DK; ++kk) {
      const int row = pair_row0<NQ>(q0, wave, nf >> 1) + (nf & 1) * 16 +
                      (lane & 15);
      bf16x8 v8 = {};
      if (row < S)
        v8 = *reinterpret_cast<const bf16x8*>(
            qp + (int64_t)row * q_rs + kk * 32 + 8 * g);
      qf[nf][kk] = v8;
    }

  const float sl2 = scale * kLog2e;
  f32x4 acc_o[DF][NQ] = {};   // O^T: d = 16*df + 4g + e, q = lane&15 (+16nf)
  float m_r[NQ], l_r[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    m_r[i] = -3.0e38f;
    l_r[i] = 0.f;
  }

  // staging registers (issue-early / write-late split): K and V rows as
  // KUN x 16B per thread each. V^T fragments are formed at read time
  // (tr_frag), so V needs no second fetch and no transposed image.
  constexpr int KUN = KB * D / 8 / NTF;
  bf16x8 krg[KUN], vrg[KUN];

  auto stage_load = [&](int kv0) {
#pragma unroll
    for (int u = 0; u < KUN; ++u) {
      const int idx = threadIdx.x + u * NTF;
      const int row = idx / (D / 8);
      const int c = (idx % (D / 8)) * 8;
      bf16x8 k8 = {}, v8 = {};   // rows >= S stay zero (pad, don't mask)
      if (kv0 + row < S) {
        k8 = *reinterpret_cast<const bf16x8*>(
            kp + (int64_t)(kv0 + row) * q_rs + c);
        v8 = *reinterpret_cast<const bf16x8*>(
            vp + (int64_t)(kv0 + row) * q_rs + c);
      }
      krg[u] = k8;
      vrg[u] = v8;
    }
  };
  auto stage_write = [&](int buf) {
    bf16_t* sK = smem + buf * BUFSZ;
    bf16_t* sV = sK + KB * D;
#pragma unroll
    for (int u = 0; u < KUN; ++u) {
      const int idx = threadIdx.x + u * NTF;
      const int row = idx / (D / 8);
      const int c = (idx % (D / 8)) * 8;
      *reinterpret_cast<bf16x8*>(sK + loff<D>(row, c)) = krg[u];
      *reinterpret_cast<bf16x8*>(sV + loff<D>(row, c)) = vrg[u];
    }
  };

  const int kv_end = causal ? min(S, q0 + 128 * NQ) : S;
  stage_load(0);
  stage_write(0);
  __syncthreads();
  int t = 0;
  for (int kv0 = 0; kv0 < kv_end; kv0 += KB, ++t) {
    const bf16_t* sK = smem + (t & 1) * BUFSZ;
    const bf16_t* sV = sK + KB * D;
    if (kv0 + KB < kv_end) stage_load(kv0 + KB);  // overlap with compute

    // wave has unmasked work (its last pair is its lowest one)
    if (!causal || kv0 <= pair_row0<NQ>(q0, wave, NQ / 2 - 1) + 31) {
#pragma unroll
      for (int hp = 0; hp < NQ / 2; ++hp) {  // sequential 32-q pairs
        const int pq0 = pair_row0<NQ>(q0, wave, hp);
        if (causal && kv0 > pq0 + 31) continue;  // pair fully masked
        // --- S^T = K Q^T: kv = 16*mi + 4g + e, q = lane&15 + 16*nf ---
        f32x4 st[4][2] = {};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < DK; ++kk)
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(
                sK + loff<D>((lane & 15) + 16 * mi, 8 * g + 32 * kk));
#pragma unroll
            for (int nf = 0; nf < 2; ++nf)
              st[mi][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  kf, qf[2 * hp + nf][kk], st[mi][nf], 0, 0, 0);
          }
        __builtin_amdgcn_s_setprio(0);
        // --- mask; online softmax (per-lane q state) on the RAW scores:
        // scale > 0, so the row max is taken before scaling and
        // p = exp2(s * (scale*log2e) - m*log2e) is one fma per element;
        // m_r / l_r / LSE stay in scaled natural-log units. Tiles fully
        // inside the causal triangle and the sequence skip the per-element
        // mask selects (wave-uniform branch) ---
        const bool inner = kv0 + KB <= pq0 && kv0 + KB <= S &&
                           pq0 + 32 <= S;
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) {
          const int nfg = 2 * hp + nf;
          const int qg = pq0 + nf * 16 + (lane & 15);
          float tmax = -3.0e38f;
          if (inner) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                tmax = fmaxf(tmax, st[mi][nf][e]);
          } else {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int kg = kv0 + mi * 16 + 4 * g + e;
                const bool masked = (causal && kg > qg) || kg >= S ||
                                    qg >= S;
                const float sv = masked ? -3.0e38f : st[mi][nf][e];
                st[mi][nf][e] = sv;
                tmax = fmaxf(tmax, sv);
              }
          }
          tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
          tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
          const float mn = fmaxf(m_r[nfg], tmax * scale);
          const float alpha = fast_exp(m_r[nfg] - mn);
          m_r[nfg] = mn;
          const float nm2 = -mn * kLog2e;
          float rs = 0.f;
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              // s*scale - mn <= 0 always; masked elements (-3e38)
              // underflow to 0
              const float p = __builtin_amdgcn_exp2f(
                  __builtin_fmaf(st[mi][nf][e], sl2, nm2));
              st[mi][nf][e] = p;
              rs += p;
            }
          rs += __shfl_xor(rs, 16, 64);
          rs += __shfl_xor(rs, 32, 64);
          l_r[nfg] = l_r[nfg] * alpha + rs;
#pragma unroll
          for (int df = 0; df < DF; ++df)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc_o[df][nfg][e] *= alpha;
        }
        // --- O^T += V^T P^T (P^T direct from accumulators) ---
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int c = 0; c < KB / 32; ++c) {
          bf16x8 pb[2];
#pragma unroll
          for (int nf = 0; nf < 2; ++nf)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              pb[nf][e] = f2bf(st[2 * c][nf][e]);
              pb[nf][e + 4] = f2bf(st[2 * c + 1][nf][e]);
            }
#pragma unroll
          for (int df = 0; df < DF; ++df) {
            const bf16x8 vfr = tr_frag<D>(sV, c, df, lane);
#pragma unroll
            for (int nf = 0; nf < 2; ++nf)
              acc_o[df][2 * hp + nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  vfr, pb[nf], acc_o[df][2 * hp + nf], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }
    if (kv0 + KB < kv_end) stage_write((t + 1) & 1);  // other buffer: no
    BAR_LDS();  // wait for readers of this buffer AND the writes above
  }

  // --- epilogue: O = O^T^T / l, write O and lse ---
#pragma unroll
  for (int nf = 0; nf < NQ; ++nf) {
    const int qg = pair_row0<NQ>(q0, wave, nf >> 1) + (nf & 1) * 16 +
                   (lane & 15);
    if (qg >= S) continue;
    const float lv = l_r[nf];
    const float inv = (lv > 0.f) ? 1.0f / lv : 0.f;
    if (g == 0)
      LSE[(int64_t)bh * S + qg] =
          (lv > 0.f) ? m_r[nf] + __logf(lv) : -3.0e38f;
#pragma unroll
    for (int df = 0; df < DF; ++df)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        op[(int64_t)qg * o_rs + 16 * df + 4 * g + e] =
            f2bf(acc_o[df][nf][e] * inv);
  }
}

}  // namespace

void attention_fwd_bf16(const void* q, const void* k, const void* v, void* o,
                        float* lse, int B, int H, int S, int D, float scale,
                        bool causal, int64_t q_bs, int64_t q_hs, int64_t q_rs,
                        int64_t o_bs, int64_t o_hs, int64_t o_rs,
                        hipStream_t stream) {
  dim3 block(NTF);
#define FWD_D(DD)                                                        \
  do {                                                                   \
    dim3 grid((S + (DD == 64 ? QBF : 256) - 1) / (DD == 64 ? QBF : 256), \
              B * H);                                                    \
    hipLaunchKernelGGL(flash_fwd_kernel<DD>, grid, block, 0, stream,     \
                       static_cast<const bf16_t*>(q),                    \
                       static_cast<const bf16_t*>(k),                    \
                       static_cast<const bf16_t*>(v),                    \
                       static_cast<bf16_t*>(o), lse, S, H, scale,        \
                       causal, q_bs, q_hs, q_rs, o_bs, o_hs, o_rs);      \
  } while (0)
  if (D == 64) FWD_D(64);
  else if (D == 128) FWD_D(128);
  else throw std::runtime_error("flash fwd: head dim must be 64 or 128");
#undef FWD_D
}

namespace {

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

// delta[bh][s] = rowsum(dO * O) (flash2 preprocess)
template <int D>
__launch_bounds__(NT) __global__
void flash_bwd_delta_kernel(const bf16_t* __restrict__ dO,
                            const bf16_t* __restrict__ O,
                            float* __restrict__ delta, int64_t rows) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int64_t nw = (int64_t)gridDim.x * (NT / WAVE);
  for (int64_t r = (int64_t)blockIdx.x * (NT / WAVE) + wid; r < rows;
       r += nw) {
    float s = 0.f;
    for (int c = lane * 8; c < D; c += WAVE * 8) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(dO + r * D + c);
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(O + r * D + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += bf2f(a[e]) * bf2f(b[e]);
    }
    s = wave_allreduce_sum(s);
    if (lane == 0) delta[r] = s;
  }
}

// Backward is TWO kernels, each free of global atomics (a single-kernel
// flash2 backward accumulates dQ with atomicAdd: 16 read-modify-write
// passes over an fp32 image dominated the measured time — see
// profiles/).
//
// Kernel A (dK/dV): one block = 64 kv rows of one (b,h); wave w owns the
// 16-kv slice kv = kv0 + 16w + (lane&15) and iterates q tiles of 64.
// Scores are computed UNtransposed, S = mfma(Q, K), so dV^T and dK^T
// consume P and dS directly from the accumulators as B-fragments via the
// MFMA k-permutation invariance against dO^T / Q^T A-operands read
// transposed from the natural tile images — P and dS never touch LDS. dK/dV accumulate transposed in
// registers across all q tiles and scatter once.
constexpr int NTA = 512;   // 8 waves; each wave owns one 16-kv slice per
                           // 128-kv slab (KBA/128 slabs per block: the q/dO
                           // tile staging+A-fragment reads amortize over
                           // every slab — the backward's staging VALU was
                           // the measured bound, profiles/flash_bwd_pmc_r2)

template <int D, int KBA = (D == 64 ? 256 : 128)>
__launch_bounds__(NTA) __global__
void flash_bwd_kv_kernel(const bf16_t* __restrict__ Q,
                         const bf16_t* __restrict__ K,
                         const bf16_t* __restrict__ V,
                         const bf16_t* __restrict__ dO,
                         const float* __restrict__ LSE,
                         const float* __restrict__ DELTA,
                         bf16_t* __restrict__ dK, bf16_t* __restrict__ dV,
                         int S, int H, float scale, bool causal,
                         int64_t q_bs, int64_t q_hs, int64_t q_rs,
                         int64_t o_bs, int64_t o_hs, int64_t o_rs) {
  constexpr int DK = D / 32;
  constexpr int DF = D / 16;
  constexpr int QT = 64;
  constexpr int NSL = KBA / 128;   // kv slabs per block
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int kv0 = blockIdx.x * KBA;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;

  const int64_t qoff = (int64_t)b * q_bs + (int64_t)h * q_hs;
  const int64_t ooff = (int64_t)b * o_bs + (int64_t)h * o_hs;
  const bf16_t* qp = Q + qoff;
  const bf16_t* kp = K + qoff;
  const bf16_t* vp = V + qoff;
  const bf16_t* dop = dO + ooff;

  // one natural image per operand: sQ/sdO are read by rows for S/dP and
  // transposed (tr_frag) for dK^T/dV^T
  __shared__ __attribute__((aligned(16))) bf16_t
      smem[KBA * D * 2 + QT * D * 2];
  bf16_t* sKb = smem;                       // [KBA][D]
  bf16_t* sVb = sKb + KBA * D;              // [KBA][D]
  bf16_t* sQ = sVb + KBA * D;               // [QT][D]
  bf16_t* sdO = sQ + QT * D;                // [QT][D]
  // per-row constants of the q tile: sNL2 = -lse*log2e (-3e38 where the
  // row has no lse) so P = exp2(S * scale*log2e + nl2) is one fma per
  // element, and delta; dS is formed without `scale`, which is applied once
  // to the dK accumulators. (Seeding the S/dP accumulators with the row
  // constants instead measured slower here: q sits on the element index,
  // so every slab pays 8 more LDS reads ahead of its MFMA chains.)
  __shared__ __attribute__((aligned(16))) float sNL2[QT], sDELTA[QT];
  const float sl2 = scale * kLog2e;

  // stage K, V tiles (fixed for the block; natural layout only)
  {
    constexpr int UN = KBA * D / 8 / NTA;
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int idx = threadIdx.x + u * NTA;
      const int row = idx / (D / 8);
      const int c = (idx % (D / 8)) * 8;
      bf16x8 kv8 = {}, vv8 = {};
      if (kv0 + row < S) {
        kv8 = *reinterpret_cast<const bf16x8*>(
            kp + (int64_t)(kv0 + row) * q_rs + c);
        vv8 = *reinterpret_cast<const bf16x8*>(
            vp + (int64_t)(kv0 + row) * q_rs + c);
      }
      *reinterpret_cast<bf16x8*>(sKb + loff<D>(row, c)) = kv8;
      *reinterpret_cast<bf16x8*>(sVb + loff<D>(row, c)) = vv8;
    }
  }
  __syncthreads();

  // K/V B-fragments are read from LDS per use (register-caching both
  // slabs' fragments pushed the kernel to 256 VGPR + scratch spills; the
  // b128 re-reads are cheaper than spilling)
  f32x4 acc_dkT[NSL][DF] = {};  // [d = 16df+4g+e][kv = slab + wave*16+l15]
  f32x4 acc_dvT[NSL][DF] = {};

  // issue-early / write-late staging registers for the Q and dO tiles
  constexpr int QUN = QT * D / 8 / NTA;
  bf16x8 qn[QUN], don[QUN];
  float lse2[QT / NTA + 1], dl2[QT / NTA + 1];

  auto tile_load = [&](int q0) {
#pragma unroll
    for (int u = 0; u < QUN; ++u) {
      const int idx = threadIdx.x + u * NTA;
      const int row = idx / (D / 8);
      const int c = (idx % (D / 8)) * 8;
      bf16x8 a = {}, b2 = {};
      if (q0 + row < S) {
        a = *reinterpret_cast<const bf16x8*>(
            qp + (int64_t)(q0 + row) * q_rs + c);
        b2 = *reinterpret_cast<const bf16x8*>(
            dop + (int64_t)(q0 + row) * o_rs + c);
      }
      qn[u] = a;
      don[u] = b2;
    }
    for (int i = threadIdx.x, s2 = 0; i < QT; i += NTA, ++s2) {
      const int qg = q0 + i;
      const float l = (qg < S) ? LSE[(int64_t)bh * S + qg] : -3.0e38f;
      lse2[s2] = (l > -1.0e38f) ? -l * kLog2e : -3.0e38f;
      dl2[s2] = (qg < S) ? DELTA[(int64_t)bh * S + qg] : 0.f;
    }
  };
  auto tile_write = [&]() {
#pragma unroll
    for (int u = 0; u < QUN; ++u) {
      const int idx = threadIdx.x + u * NTA;
      const int row = idx / (D / 8);
      const int c = (idx % (D / 8)) * 8;
      *reinterpret_cast<bf16x8*>(sQ + loff<D>(row, c)) = qn[u];
      *reinterpret_cast<bf16x8*>(sdO + loff<D>(row, c)) = don[u];
    }
    for (int i = threadIdx.x, s2 = 0; i < QT; i += NTA, ++s2) {
      sNL2[i] = lse2[s2];
      sDELTA[i] = dl2[s2];
    }
  };

  const int q_start = causal ? (kv0 / QT) * QT : 0;
  tile_load(q_start);
  tile_write();
  __syncthreads();
  for (int q0 = q_start; q0 < S; q0 += QT) {
    if (q0 + QT < S) tile_load(q0 + QT);  // overlap with compute

#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
      // this wave's 16-kv slice lies wholly above the diagonal of the q
      // tile: every P and dS would be zero (wave-uniform; no barrier in
      // the slab body)
      if (causal && kv0 + sl * 128 + wave * 16 > q0 + QT - 1) continue;
      // S = Q K^T ; dP = dO V^T  — C-frags: q = 16mi+4g+e, kv = lane&15
      f32x4 st[4] = {};
      f32x4 dpt[4] = {};
#pragma unroll
      for (int kk = 0; kk < DK; ++kk) {
        const bf16x8 kfr = *reinterpret_cast<const bf16x8*>(
            sKb + loff<D>(sl * 128 + wave * 16 + (lane & 15),
                          8 * g + 32 * kk));
        const bf16x8 vfr = *reinterpret_cast<const bf16x8*>(
            sVb + loff<D>(sl * 128 + wave * 16 + (lane & 15),
                          8 * g + 32 * kk));
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const bf16x8 qa = *reinterpret_cast<const bf16x8*>(
              sQ + loff<D>(16 * mi + (lane & 15), 8 * g + 32 * kk));
          st[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, kfr,
                                                           st[mi], 0, 0, 0);
          const bf16x8 da = *reinterpret_cast<const bf16x8*>(
              sdO + loff<D>(16 * mi + (lane & 15), 8 * g + 32 * kk));
          dpt[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              da, vfr, dpt[mi], 0, 0, 0);
        }
      }

      // P and dS (elementwise); kv fixed per lane, q varies per element.
      // Inner tiles skip the per-element mask selects (wave-uniform).
      const int kvb = kv0 + sl * 128;
      const int kvg = kvb + wave * 16 + (lane & 15);
      const bool winner = (!causal || kvb + wave * 16 + 15 < q0) &&
                          q0 + QT <= S && kvb + 128 <= S;
      if (winner) {
        f32x4 nl2v[4], dlv[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          nl2v[mi] = *reinterpret_cast<const f32x4*>(sNL2 + 16 * mi + 4 * g);
          dlv[mi] = *reinterpret_cast<const f32x4*>(sDELTA + 16 * mi + 4 * g);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float pt = __builtin_amdgcn_exp2f(
                __builtin_fmaf(st[mi][e], sl2, nl2v[mi][e]));
            st[mi][e] = pt;                              // now P
            dpt[mi][e] = pt * (dpt[mi][e] - dlv[mi][e]); // now dS / scale
          }
      } else {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int qrow = 16 * mi + 4 * g + e;
            const int qg = q0 + qrow;
            const float nl2 = sNL2[qrow];
            const float dl = sDELTA[qrow];
            const bool valid = qg < S && kvg < S && (!causal || kvg <= qg) &&
                               nl2 > -1.0e38f;
            const float arg =
                valid ? __builtin_fmaf(st[mi][e], sl2, nl2) : -3.0e38f;
            const float pt = __builtin_amdgcn_exp2f(arg);  // select, not branch
            st[mi][e] = pt;                        // now P
            dpt[mi][e] = pt * (dpt[mi][e] - dl);   // now dS / scale
          }
      }

      // dV^T += dO^T P and dK^T += Q^T dS (both k-permuted B from regs)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < QT / 32; ++c) {
        bf16x8 pb, db;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pb[e] = f2bf(st[2 * c][e]);
          pb[e + 4] = f2bf(st[2 * c + 1][e]);
          db[e] = f2bf(dpt[2 * c][e]);
          db[e + 4] = f2bf(dpt[2 * c + 1][e]);
        }
#pragma unroll
        for (int df = 0; df < DF; ++df) {
          const bf16x8 afr = tr_frag<D>(sdO, c, df, lane);
          const bf16x8 qfr = tr_frag<D>(sQ, c, df, lane);
          acc_dvT[sl][df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afr, pb, acc_dvT[sl][df], 0, 0, 0);
          acc_dkT[sl][df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qfr, db, acc_dkT[sl][df], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
    BAR_LDS();  // sQ/sdO reads retired
    if (q0 + QT < S) {
      tile_write();
      BAR_LDS();  // next tile's images visible
    }
  }

  // write dK, dV (transposed-accumulator scatter: kv = wave's lane slice)
#pragma unroll
  for (int sl = 0; sl < NSL; ++sl) {
    const int kvg = kv0 + sl * 128 + wave * 16 + (lane & 15);
    if (kvg < S) {
#pragma unroll
      for (int df = 0; df < DF; ++df) {
        bf16x4 kv4, vv4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          kv4[e] = f2bf(acc_dkT[sl][df][e] * scale);
          vv4[e] = f2bf(acc_dvT[sl][df][e]);
        }
        const int64_t off = qoff + (int64_t)kvg * q_rs + 16 * df + 4 * g;
        *reinterpret_cast<bf16x4*>(dK + off) = kv4;
        *reinterpret_cast<bf16x4*>(dV + off) = vv4;
      }
    }
  }
}

// Kernel B (dQ): forward-shaped — one block = 128 q rows, wave w owns 32 q
// columns, iterates kv tiles; dQ accumulates TRANSPOSED in registers
// ([d][q], q = lane&15 like the fwd O^T accumulator) with dS^T consumed
// straight from the accumulators (k-permutation) against K^T read
// transposed from the natural K image — no LDS scatter, no atomics, bf16 output written
// directly (strided; serves the packed-qkv layout too).
constexpr int NTB = 512;   // 8 waves; D=64 blocks take 512 q (two
                           // sequential 32-q pairs per wave — the same
                           // staging-amortization as fwd/bwd-kv), D=128
                           // keeps 256 (register budget)
constexpr int QBB = 256;   // D=128 block size; D=64 uses 128*NQ

template <int D, int NQ = (D == 64 ? 4 : 2)>
__launch_bounds__(NTB) __global__
void flash_bwd_dq_kernel(const bf16_t* __restrict__ Q,
                         const bf16_t* __restrict__ K,
                         const bf16_t* __restrict__ V,
                         const bf16_t* __restrict__ dO,
                         const float* __restrict__ LSE,
                         const float* __restrict__ DELTA,
                         bf16_t* __restrict__ dQ, int S, int H, float scale,
                         bool causal, int64_t q_bs, int64_t q_hs,
                         int64_t q_rs, int64_t o_bs, int64_t o_hs,
                         int64_t o_rs) {
  constexpr int DK = D / 32;
  constexpr int DF = D / 16;
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int q0 = blockIdx.x * (128 * NQ);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;

  const int64_t qoff = (int64_t)b * q_bs + (int64_t)h * q_hs;
  const int64_t ooff = (int64_t)b * o_bs + (int64_t)h * o_hs;
  const bf16_t* qp = Q + qoff;
  const bf16_t* kp = K + qoff;
  const bf16_t* vp = V + qoff;
  const bf16_t* dop = dO + ooff;
  bf16_t* dqp = dQ + qoff;

  __shared__ __attribute__((aligned(16))) bf16_t smem[KB * D * 2];
  bf16_t* sK = smem;                    // [KB][D]; rows for S^T, tr_frag
                                        // columns for the dQ^T A-operand
  bf16_t* sV = smem + KB * D;           // [KB][D]

  // Q and dO B-fragments + per-lane row constants (block-constant). q is
  // the lane here, so the constants fold into one fma per element
  // (P = exp2(s * scale*log2e + nl2_r), nl2_r = -lse*log2e, -3e38 where the
  // row has no lse); seeding the MFMA accumulators with them costs 4
  // registers per constant and spilled. `scale` is applied once to the dQ
  // accumulators.
  const float sl2 = scale * kLog2e;
  bf16x8 qf[NQ][DK], dof[NQ][DK];
  float nl2_r[NQ], dl_r[NQ];
#pragma unroll
  for (int nf = 0; nf < NQ; ++nf) {
    const int row = pair_row0<NQ>(q0, wave, nf >> 1) + (nf & 1) * 16 +
                    (lane & 15);
    const float l = (row < S) ? LSE[(int64_t)bh * S + row] : -3.0e38f;
    nl2_r[nf] = (l > -1.0e38f) ? -l * kLog2e : -3.0e38f;
    dl_r[nf] = (row < S) ? DELTA[(int64_t)bh * S + row] : 0.f;
#pragma unroll
    for (int kk = 0; kk < DK; ++kk) {
      bf16x8 a = {}, b8 = {};
      if (row < S) {
        a = *reinterpret_cast<const bf16x8*>(
            qp + (int64_t)row * q_rs + kk * 32 + 8 * g);
        b8 = *reinterpret_cast<const bf16x8*>(
            dop + (int64_t)row * o_rs + kk * 32 + 8 * g);
      }
      qf[nf][kk] = a;
      dof[nf][kk] = b8;
    }
  }

  f32x4 acc_dq[DF][NQ] = {};  // dQ^T: d = 16df+4g+e, q = lane&15 (+16nf)

  // staging registers: K,V rows (16B each)
  constexpr int KUN = KB * D / 8 / NTB;
  bf16x8 krg[KUN], vrg[KUN];

  auto stage_load = [&](int kv0) {
#pragma unroll
    for (int u = 0; u < KUN; ++u) {
      const int idx = threadIdx.x + u * NTB;
      const int row = idx / (D / 8);
      const int c = (idx % (D / 8)) * 8;
      bf16x8 kv8 = {}, vv8 = {};
      if (kv0 + row < S) {
        kv8 = *reinterpret_cast<const bf16x8*>(
            kp + (int64_t)(kv0 + row) * q_rs + c);
        vv8 = *reinterpret_cast<const bf16x8*>(
            vp + (int64_t)(kv0 + row) * q_rs + c);
      }
      krg[u] = kv8;
      vrg[u] = vv8;
    }
  };
  auto stage_write = [&]() {
#pragma unroll
    for (int u = 0; u < KUN; ++u) {
      const int idx = threadIdx.x + u * NTB;
      const int row = idx / (D / 8);
      const int c = (idx % (D / 8)) * 8;
      *reinterpret_cast<bf16x8*>(sK + loff<D>(row, c)) = krg[u];
      *reinterpret_cast<bf16x8*>(sV + loff<D>(row, c)) = vrg[u];
    }
  };

  const int kv_end = causal ? min(S, q0 + 128 * NQ) : S;
  stage_load(0);
  stage_write();
  __syncthreads();
  for (int kv0 = 0; kv0 < kv_end; kv0 += KB) {
    if (kv0 + KB < kv_end) stage_load(kv0 + KB);

    if (!causal || kv0 <= pair_row0<NQ>(q0, wave, NQ / 2 - 1) + 31) {
#pragma unroll
     for (int hp = 0; hp < NQ / 2; ++hp) {
      const int pq0 = pair_row0<NQ>(q0, wave, hp);
      if (causal && kv0 > pq0 + 31) continue;
      // per 16-kv block: S^T = K Q^T and dP^T = V dO^T, then dS^T packed
      // to bf16 immediately (keeps only two f32x4 accumulator pairs live
      // at a time — register pressure gates a second wave per SIMD)
      const bool inner = kv0 + KB <= pq0 && kv0 + KB <= S && pq0 + 32 <= S;
      bf16x4 dsb[4][2];   // dS^T bf16: kv = 16mi+4g+e, q = lane&15+16nf
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        f32x4 st[2] = {};
        f32x4 dpt[2] = {};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < DK; ++kk) {
          const bf16x8 ka = *reinterpret_cast<const bf16x8*>(
              sK + loff<D>((lane & 15) + 16 * mi, 8 * g + 32 * kk));
          const bf16x8 va = *reinterpret_cast<const bf16x8*>(
              sV + loff<D>((lane & 15) + 16 * mi, 8 * g + 32 * kk));
#pragma unroll
          for (int nf = 0; nf < 2; ++nf) {
            st[nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                ka, qf[2 * hp + nf][kk], st[nf], 0, 0, 0);
            dpt[nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                va, dof[2 * hp + nf][kk], dpt[nf], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) {
          const int nfg = 2 * hp + nf;
          const int qg = pq0 + nf * 16 + (lane & 15);
          if (inner) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float pt = __builtin_amdgcn_exp2f(
                  __builtin_fmaf(st[nf][e], sl2, nl2_r[nfg]));
              dsb[mi][nf][e] =
                  f2bf(pt * (dpt[nf][e] - dl_r[nfg]));   // dS / scale
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int kg = kv0 + 16 * mi + 4 * g + e;
              const bool valid = qg < S && kg < S &&
                                 (!causal || kg <= qg) &&
                                 nl2_r[nfg] > -1.0e38f;
              const float arg =
                  valid ? __builtin_fmaf(st[nf][e], sl2, nl2_r[nfg])
                        : -3.0e38f;
              const float pt = __builtin_amdgcn_exp2f(arg);
              dsb[mi][nf][e] =
                  f2bf(pt * (dpt[nf][e] - dl_r[nfg]));   // dS / scale
            }
          }
        }
      }
      // dQ^T += K^T dS^T (k-permuted B straight from the accumulators)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < KB / 32; ++c) {
        bf16x8 db[2];
#pragma unroll
        for (int nf = 0; nf < 2; ++nf)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            db[nf][e] = dsb[2 * c][nf][e];
            db[nf][e + 4] = dsb[2 * c + 1][nf][e];
          }
#pragma unroll
        for (int df = 0; df < DF; ++df) {
          const bf16x8 kfr = tr_frag<D>(sK, c, df, lane);
#pragma unroll
          for (int nf = 0; nf < 2; ++nf)
            acc_dq[df][2 * hp + nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                kfr, db[nf], acc_dq[df][2 * hp + nf], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
     }
    }
    BAR_LDS();
    if (kv0 + KB < kv_end) {
      stage_write();
      BAR_LDS();
    }
  }

  // write dQ (transposed-accumulator scatter, bf16, strided layout)
#pragma unroll
  for (int nf = 0; nf < NQ; ++nf) {
    const int qg = pair_row0<NQ>(q0, wave, nf >> 1) + (nf & 1) * 16 +
                   (lane & 15);
    if (qg >= S) continue;
#pragma unroll
    for (int df = 0; df < DF; ++df) {
      bf16x4 v4;
#pragma unroll
      for (int e = 0; e < 4; ++e) v4[e] = f2bf(acc_dq[df][nf][e] * scale);
      *reinterpret_cast<bf16x4*>(
          dqp + (int64_t)qg * q_rs + 16 * df + 4 * g) = v4;
    }
  }
}


// delta kernel needs contiguous dO/O rows: the host passes per-(b,h)
// strided views by iterating bh in the kernel via strides
// each row of D elements is handled by D/8 lanes (one bf16x8 each), so a
// 64-lane wave covers 64*8/D rows per iteration (8 rows at D=64) — the
// whole wave's 1 KiB load capacity is used every cycle.
template <int D>
__global__ void flash_bwd_delta_strided_kernel(
    const bf16_t* __restrict__ dO, const bf16_t* __restrict__ O,
    float* __restrict__ delta, int H, int S, int64_t o_bs, int64_t o_hs,
    int64_t o_rs) {
  constexpr int LPR = D / 8;              // lanes per row
  constexpr int RPW = WAVE / LPR;         // rows per wave per iteration
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int sub = lane / LPR;             // row slot within the wave
  const int c = (lane % LPR) * 8;
  const int64_t nr = (int64_t)gridDim.x * (NT / WAVE) * RPW;
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int64_t off = (int64_t)b * o_bs + (int64_t)h * o_hs;
  for (int64_t r0 = ((int64_t)blockIdx.x * (NT / WAVE) + wid) * RPW;
       r0 < S; r0 += nr) {
    const int64_t r = r0 + sub;
    float s = 0.f;
    if (r < S) {
      const bf16x8 a =
          *reinterpret_cast<const bf16x8*>(dO + off + r * o_rs + c);
      const bf16x8 bb =
          *reinterpret_cast<const bf16x8*>(O + off + r * o_rs + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += bf2f(a[e]) * bf2f(bb[e]);
    }
    // reduce across the LPR lanes of each row slot
#pragma unroll
    for (int d2 = 1; d2 < LPR; d2 <<= 1) s += __shfl_xor(s, d2, 64);
    if (r < S && (lane % LPR) == 0) delta[(int64_t)bh * S + r] = s;
  }
}

}  // namespace



void attention_bwd_bf16(const void* q, const void* k, const void* v,
                        const void* o, const void* dout, const float* lse,
                        float* delta, void* dq, void* dk, void* dv,
                        int B, int H, int S, int D, float scale, bool causal,
                        int64_t q_bs, int64_t q_hs, int64_t q_rs,
                        int64_t o_bs, int64_t o_hs, int64_t o_rs,
                        hipStream_t stream) {
  dim3 block(NT);
#define BWD_D(DD)                                                            \
  do {                                                                       \
    dim3 dgrid((S / 4 + (NT / WAVE) - 1) / (NT / WAVE) > 256                 \
                   ? 256 : (S + 3) / 4, B * H);                              \
    hipLaunchKernelGGL(flash_bwd_delta_strided_kernel<DD>, dgrid, block, 0,  \
                       stream, static_cast<const bf16_t*>(dout),             \
                       static_cast<const bf16_t*>(o), delta, H, S, o_bs,     \
                       o_hs, o_rs);                                          \
    dim3 kgrid((S + (DD == 64 ? 255 : 127)) / (DD == 64 ? 256 : 128),       \
               B * H);                                                       \
    hipLaunchKernelGGL(flash_bwd_kv_kernel<DD>, kgrid, dim3(512), 0, stream, \
                       static_cast<const bf16_t*>(q),                        \
                       static_cast<const bf16_t*>(k),                        \
                       static_cast<const bf16_t*>(v),                        \
                       static_cast<const bf16_t*>(dout), lse, delta,         \
                       static_cast<bf16_t*>(dk), static_cast<bf16_t*>(dv),   \
                       S, H, scale, causal, q_bs, q_hs, q_rs, o_bs, o_hs,    \
                       o_rs);                                                \
    dim3 qgrid((S + (DD == 64 ? 511 : 255)) / (DD == 64 ? 512 : 256),       \
               B * H);                                                       \
    hipLaunchKernelGGL(flash_bwd_dq_kernel<DD>, qgrid, dim3(NTB), 0, stream, \
                       static_cast<const bf16_t*>(q),                        \
                       static_cast<const bf16_t*>(k),                        \
                       static_cast<const bf16_t*>(v),                        \
                       static_cast<const bf16_t*>(dout), lse, delta,         \
                       static_cast<bf16_t*>(dq), S, H, scale, causal, q_bs,  \
                       q_hs, q_rs, o_bs, o_hs, o_rs);                        \
  } while (0)
  if (D == 64) BWD_D(64);
  else if (D == 128) BWD_D(128);
  else throw std::runtime_error("flash bwd: head dim must be 64 or 128");
#undef BWD_D
}
}  // namespace tepdist
