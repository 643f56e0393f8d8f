// Multi-query-row ("chunked prefill") attention over a KV cache for gfx950:
// a chunk of T tokens per batch row, starting at the device-side position
// p0[b], attends cache rows 0 .. p0 + t of its K/V head. Forward only.
// docs/KERNELS.md "Prefill attention over the cache" has the discussion.
//
// Two launches on one stream:
//
//   prefill_append_kernel   one 16-byte lane per (b, t, kv head, 8 columns):
//     rotates the chunk's K rows at p0 + t (partner vector i ^ D/2 fetched
//     with a second global load, angles from rope_common.h), rounds once to
//     bf16 and stores K and V into cache rows p0 .. p0 + T - 1 with 16-byte
//     vector stores. The attention kernel then reads every key from the
//     cache: the ordering between the two is the stream's, not something
//     workgroups of one launch have to agree on.
//
//   prefill_attn_kernel     one 256-thread block per (q tile, kv head, b),
//     grid (ceil(T*G / 128), Hkv, B), static. A block owns 128 MFMA rows
//     r = t_local * G + g: 128 / G consecutive tokens times the G query
//     heads of the group, token-major, so every staged K/V row serves the
//     whole group. The schedule is the flash forward's (attention.hip):
//     S^T = mfma(K, Q) puts the query row in the lane index, the online
//     softmax state is per lane with two shfl_xor per reduction, P feeds
//     the second MFMA from the accumulators (k-permutation invariance)
//     against V^T read through tr_frag<D>. K/V tiles of 64 cache rows are
//     fetched with 16-byte row loads into one swizzled natural image each,
//     double-buffered, one LDS-only barrier per tile, shared by the four
//     waves (32 rows each).
//
// Position: p0 = clamp(pos[b], 0, S_max - T), made scalar with
// readfirstlane. Row r sees key j iff j <= p0 + t(r). The kv loop stops at
// the tile holding p0 + t_max of the block; rows past that key are never
// loaded (staging lanes past it re-load that last row and are switched off
// by selects on score and probability), so whatever the cache holds above
// p0 + T - 1 has no effect. "Minus infinity" is finite. A wave skips tiles
// wholly above its rows' diagonal and takes a mask-free path on tiles wholly
// below it; both tests are wave-uniform and no barrier sits inside them.
// Q rows >= T*G are zero-padded, never masked, and not stored.
//
// No split over KV, no atomics, no workspace: results repeat bit for bit.

#include <cmath>
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "lds_frag.h"
#include "mx_kv.h"
#include "rope_common.h"

namespace tepdist {

namespace {

constexpr int NT = 256;
constexpr int QB = 128;  // MFMA rows (token x group member) per block
constexpr int KB = 64;   // cache rows per tile
constexpr float NEG = -3.0e38f;
constexpr float kLog2e = 1.4426950408889634f;

// execution barrier with LDS visibility only (no vmcnt drain): the next
// tile's global loads stay in flight across it
#define PA_BAR_LDS()                                     \
  do {                                                   \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
    __builtin_amdgcn_s_barrier();                        \
  } while (0)

DEV_INLINE int clamp_p0(const int64_t* pos, int b, int pos_stride, int S_max,
                        int T) {
  int64_t p = pos[(int64_t)b * pos_stride];
  p = p < 0 ? 0 : p;
  p = p > S_max - T ? S_max - T : p;  // host: T <= S_max
  return (int)p;
}

// ---------------------------------------------------------------------------
// append (+ rotate)
// ---------------------------------------------------------------------------

// KV8: the caches are MXFP8 (ops/mx.py MXCache). k_cache / v_cache then point
// at the e4m3 codes with (c_bs, c_hs, c_rs) in bytes, k_sc / v_sc at the e8m0
// scale bytes with (s_bs, s_hs, s_rs); the row is rotated and rounded as
// below, then quantized in registers by mx_quantize's rule (mxkv_quant8: the
// four lanes of a quad hold one block; LPR is a multiple of 4, so a quad is
// wholly inside or outside the problem) and stored as 8 code bytes per lane
// and one scale byte per quad.
template <int D, bool ROPE, bool KV8 = false>
__launch_bounds__(NT) __global__
void prefill_append_kernel(const bf16_t* __restrict__ k_new,
                           const bf16_t* __restrict__ v_new,
                           bf16_t* __restrict__ k_cache,
                           bf16_t* __restrict__ v_cache,
                           const int64_t* __restrict__ pos, int pos_stride,
                           int B, int T, int Hkv, int S_max,
                           float neg2_over_d, float ltheta, int64_t n_bs,
                           int64_t n_ts, int64_t n_hs, int64_t c_bs,
                           int64_t c_hs, int64_t c_rs,
                           uint8_t* __restrict__ k_sc = nullptr,
                           uint8_t* __restrict__ v_sc = nullptr,
                           int64_t s_bs = 0, int64_t s_hs = 0,
                           int64_t s_rs = 0) {
  constexpr int LPR = D / 8;  // lanes per row
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (int64_t)B * T * Hkv * LPR) return;
  const int col = (int)(idx % LPR) * 8;
  const int64_t row = idx / LPR;
  const int hk = (int)(row % Hkv);
  const int t = (int)((row / Hkv) % T);
  const int b = (int)(row / Hkv / T);
  const int p = clamp_p0(pos, b, pos_stride, S_max, T) + t;  // < S_max

  const int64_t src = b * n_bs + t * n_ts + hk * n_hs;
  const int64_t dst = b * c_bs + hk * c_hs + (int64_t)p * c_rs + col;
  bf16x8 k8 = *reinterpret_cast<const bf16x8*>(k_new + src + col);
  const bf16x8 v8 = *reinterpret_cast<const bf16x8*>(v_new + src + col);
  if (ROPE) {
    const bf16x8 x8 = k8;
    const bf16x8 xp =
        *reinterpret_cast<const bf16x8*>(k_new + src + (col ^ (D / 2)));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float sn, cs;
      rope_sincos(p, (col + e) & (D / 2 - 1), neg2_over_d, ltheta, &sn, &cs);
      const float x = bf2f(x8[e]), y = bf2f(xp[e]);
      // rotate-half: first half x1 cos - x2 sin, second x2 cos + x1 sin
      k8[e] = f2bf(col < D / 2 ? x * cs - y * sn : x * cs + y * sn);
    }
  }
  if constexpr (KV8) {
    const u32x4 kw = __builtin_bit_cast(u32x4, k8);
    const u32x4 vw = __builtin_bit_cast(u32x4, v8);
    unsigned kq0, kq1, kqb, vq0, vq1, vqb;
    mxkv_quant8(kw[0], kw[1], kw[2], kw[3], kq0, kq1, kqb);
    mxkv_quant8(vw[0], vw[1], vw[2], vw[3], vq0, vq1, vqb);
    *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(k_cache) + dst) =
        make_uint2(kq0, kq1);
    *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(v_cache) + dst) =
        make_uint2(vq0, vq1);
    if ((threadIdx.x & 3) == 0) {
      const int64_t sd =
          b * s_bs + hk * s_hs + (int64_t)p * s_rs + (col >> 5);
      k_sc[sd] = (uint8_t)kqb;
      v_sc[sd] = (uint8_t)vqb;
    }
  } else {
    *reinterpret_cast<bf16x8*>(k_cache + dst) = k8;
    *reinterpret_cast<bf16x8*>(v_cache + dst) = v8;
  }
}

// ---------------------------------------------------------------------------
// attention
// ---------------------------------------------------------------------------

// lg = log2(G). Row r of the (b, kv head) problem is token r >> lg, group
// member r & (G - 1), i.e. query head hk * G + (r & (G - 1)).
// KV8: Kc / Vc point at e4m3 codes with byte strides, Ks / Vs at the scale
// bytes (see prefill_append_kernel). Only the staging differs: stage_load
// fetches 8 code bytes and the block's scale byte per slot, stage_write
// dequantizes them (dq_fp8, exact) into the same swizzled bf16 images.
template <int D, bool ROPE, bool KV8 = false>
__launch_bounds__(NT) __global__
void prefill_attn_kernel(const bf16_t* __restrict__ Q,
                         const bf16_t* __restrict__ Kc,
                         const bf16_t* __restrict__ Vc,
                         const int64_t* __restrict__ pos, int pos_stride,
                         bf16_t* __restrict__ O, int T, int H, int lg,
                         int S_max, float scale, float neg2_over_d,
                         float ltheta, int64_t q_bs, int64_t q_ts,
                         int64_t q_hs, int64_t c_bs, int64_t c_hs,
                         int64_t c_rs,
                         const uint8_t* __restrict__ Ks = nullptr,
                         const uint8_t* __restrict__ Vs = nullptr,
                         int64_t s_bs = 0, int64_t s_hs = 0,
                         int64_t s_rs = 0) {
  constexpr int DK = D / 32;  // k-chunks per d-contraction fragment
  constexpr int DF = D / 16;  // d row fragments of O^T
  const int G = 1 << lg;
  const int TG = T << lg;
  const int hk = blockIdx.y, b = blockIdx.z;
  const int r0 = blockIdx.x * QB;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int gl = lane >> 4;

  const int p0 = __builtin_amdgcn_readfirstlane(
      clamp_p0(pos, b, pos_stride, S_max, T));
  // keys the block's last token sees: the kv loop's trip count
  const int kv_end = p0 + min(T - 1, (r0 + QB - 1) >> lg) + 1;

  // this wave's 32 rows: token range, and whether any row exists at all
  const int wr0 = r0 + 32 * wave;
  const bool live = wr0 < TG;
  const int tw_lo = wr0 >> lg;
  const int tw_hi = min(T - 1, (wr0 + 31) >> lg);

  // this (b, kv head)'s planes: bf16 rows, or (KV8, byte strides) codes
  const bf16_t* kp = KV8 ? nullptr : Kc + b * c_bs + hk * c_hs;
  const bf16_t* vp = KV8 ? nullptr : Vc + b * c_bs + hk * c_hs;
  const uint8_t* kq = reinterpret_cast<const uint8_t*>(Kc) +
                      (KV8 ? b * c_bs + hk * c_hs : 0);
  const uint8_t* vq = reinterpret_cast<const uint8_t*>(Vc) +
                      (KV8 ? b * c_bs + hk * c_hs : 0);

  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * 2 * KB * D];
  constexpr int BUFSZ = 2 * KB * D;  // K and V, both natural [KB][D]

  // Q fragments (B operand of S^T = K Q^T): nf-th 16-row group, kk-th 32-d
  // chunk; lane (gl, i) holds row i, columns 32 kk + 8 gl .. + 7. The RoPE
  // partner of chunk kk is chunk kk ^ (DK / 2) of the same lane, so the
  // rotation needs no second load.
  bf16x8 qf[2][DK];
  int qlim[2];  // last key the lane's row sees
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    const int r = wr0 + 16 * nf + (lane & 15);
    const int t = min(r >> lg, T - 1);
    qlim[nf] = p0 + t;
    const bf16_t* qp = Q + b * q_bs + (int64_t)t * q_ts +
                       (int64_t)(hk * G + (r & (G - 1))) * q_hs + 8 * gl;
#pragma unroll
    for (int kk = 0; kk < DK; ++kk) {
      bf16x8 v8 = {};
      if (r < TG) v8 = *reinterpret_cast<const bf16x8*>(qp + 32 * kk);
      qf[nf][kk] = v8;
    }
    if (ROPE) {
#pragma unroll
      for (int kk = 0; kk < DK / 2; ++kk) {
        const bf16x8 x1 = qf[nf][kk], x2 = qf[nf][kk + DK / 2];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float sn, cs;
          rope_sincos(p0 + t, 32 * kk + 8 * gl + e, neg2_over_d, ltheta, &sn,
                      &cs);
          const float a = bf2f(x1[e]), c = bf2f(x2[e]);
          qf[nf][kk][e] = f2bf(a * cs - c * sn);
          qf[nf][kk + DK / 2][e] = f2bf(c * cs + a * sn);
        }
      }
    }
  }

  const float sl2 = scale * kLog2e;
  f32x4 acc_o[DF][2] = {};  // O^T: d = 16 df + 4 gl + e, row = lane & 15
  float m_r[2] = {NEG, NEG}, l_r[2] = {0.f, 0.f};

  // staging registers (issue early, write late): KUN x 16 B of K and of V
  // per thread. Rows at or past kv_end re-load row kv_end - 1.
  constexpr int KUN = KB * D / 8 / NT;
  bf16x8 krg[KUN], vrg[KUN];
  // KV8: 8 codes and the block's scale byte per slot; a clamped row re-loads
  // the last visible row's codes and scales
  uint2 kcd[KUN], vcd[KUN];
  unsigned ksc[KUN], vsc[KUN];
  auto stage_load = [&](int kv0) {
#pragma unroll
    for (int u = 0; u < KUN; ++u) {
      const int idx = threadIdx.x + u * NT;
      const int c = (idx % (D / 8)) * 8;
      int j = kv0 + idx / (D / 8);
      j = j < kv_end ? j : kv_end - 1;
      if constexpr (KV8) {
        const int64_t so = b * s_bs + hk * s_hs + (int64_t)j * s_rs + (c >> 5);
        kcd[u] = *reinterpret_cast<const uint2*>(kq + (int64_t)j * c_rs + c);
        vcd[u] = *reinterpret_cast<const uint2*>(vq + (int64_t)j * c_rs + c);
        ksc[u] = Ks[so];
        vsc[u] = Vs[so];
      } else {
        krg[u] = *reinterpret_cast<const bf16x8*>(kp + (int64_t)j * c_rs + c);
        vrg[u] = *reinterpret_cast<const bf16x8*>(vp + (int64_t)j * c_rs + c);
      }
    }
  };
  auto stage_write = [&](int buf) {
    bf16_t* sK = smem + buf * BUFSZ;
    bf16_t* sV = sK + KB * D;
#pragma unroll
    for (int u = 0; u < KUN; ++u) {
      const int idx = threadIdx.x + u * NT;
      const int row = idx / (D / 8);
      const int c = (idx % (D / 8)) * 8;
      if constexpr (KV8) {
        krg[u] = dq_fp8(kcd[u].x, kcd[u].y, mx_scale(ksc[u]));
        vrg[u] = dq_fp8(vcd[u].x, vcd[u].y, mx_scale(vsc[u]));
      }
      *reinterpret_cast<bf16x8*>(sK + loff<D>(row, c)) = krg[u];
      *reinterpret_cast<bf16x8*>(sV + loff<D>(row, c)) = vrg[u];
    }
  };

  stage_load(0);
  stage_write(0);
  __syncthreads();
  int it = 0;
  for (int kv0 = 0; kv0 < kv_end; kv0 += KB, ++it) {
    const bf16_t* sK = smem + (it & 1) * BUFSZ;
    const bf16_t* sV = sK + KB * D;
    if (kv0 + KB < kv_end) stage_load(kv0 + KB);  // overlaps the compute

    if (live && kv0 <= p0 + tw_hi) {  // wave-uniform: some row sees a key
      // --- S^T = K Q^T: key = 16 mi + 4 gl + e, row = lane & 15 + 16 nf ---
      f32x4 st[4][2] = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < DK; ++kk)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(
              sK + loff<D>((lane & 15) + 16 * mi, 8 * gl + 32 * kk));
#pragma unroll
          for (int nf = 0; nf < 2; ++nf)
            st[mi][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                kf, qf[nf][kk], st[mi][nf], 0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);
      // --- online softmax on the raw scores (scale > 0: the max is taken
      // before scaling, p = exp2 of one fma). A tile every row of the wave
      // sees whole skips the selects (wave-uniform) ---
      const bool inner = kv0 + KB <= p0 + tw_lo + 1;
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        const int ql = qlim[nf] - kv0 - 4 * gl;  // masked: 16 mi + e > ql
        float tmax = NEG;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (!inner)
              st[mi][nf][e] = 16 * mi + e > ql ? NEG : st[mi][nf][e];
            tmax = fmaxf(tmax, st[mi][nf][e]);
          }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        // key 0 is in the first tile and every row sees it, so mn is a real
        // score from the first tile on
        const float mn = fmaxf(m_r[nf], tmax * scale);
        const float alpha = __builtin_amdgcn_exp2f((m_r[nf] - mn) * kLog2e);
        m_r[nf] = mn;
        const float nm2 = -mn * kLog2e;
        float rs = 0.f;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float p = __builtin_amdgcn_exp2f(
                __builtin_fmaf(st[mi][nf][e], sl2, nm2));
            if (!inner) p = 16 * mi + e > ql ? 0.f : p;
            st[mi][nf][e] = p;
            rs += p;
          }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l_r[nf] = l_r[nf] * alpha + rs;
#pragma unroll
        for (int df = 0; df < DF; ++df)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc_o[df][nf][e] *= alpha;
      }
      // --- O^T += V^T P^T (P^T straight from the accumulators) ---
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
            acc_o[df][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                vfr, pb[nf], acc_o[df][nf], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
    if (kv0 + KB < kv_end) stage_write((it + 1) & 1);  // the other buffer
    PA_BAR_LDS();  // readers of this buffer done, writes above visible
  }

  // --- epilogue: out[b, t, hk*G + g, :] = O^T^T / l, 8 bytes per lane ---
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    const int r = wr0 + 16 * nf + (lane & 15);
    if (r >= TG) continue;
    const float inv = 1.0f / l_r[nf];  // key 0 is always seen: l > 0
    bf16_t* op = O + (((int64_t)b * T + (r >> lg)) * H + hk * G +
                      (r & (G - 1))) * D + 4 * gl;
#pragma unroll
    for (int df = 0; df < DF; ++df) {
      bf16x4 o4;
#pragma unroll
      for (int e = 0; e < 4; ++e) o4[e] = f2bf(acc_o[df][nf][e] * inv);
      *reinterpret_cast<bf16x4*>(op + 16 * df) = o4;
    }
  }
}

bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// checks shared by the bf16 and the MXFP8 cache entry points
int check_problem(int B, int T, int H, int Hkv, int S_max, int D, float scale,
                  bool rope, float rope_theta, int pos_stride,
                  const void* k_new, const void* v_new) {
  if (D != 64 && D != 128)
    throw std::runtime_error("prefill_attention: head dim must be 64 or 128");
  if (B < 1 || B > 65535 || Hkv < 1 || Hkv > 65535 || T < 1 || S_max < 1)
    throw std::runtime_error("prefill_attention: bad B/Hkv/T/S_max");
  if (T > S_max)
    throw std::runtime_error("prefill_attention: chunk longer than the cache");
  if (H < 1 || H % Hkv != 0)
    throw std::runtime_error("prefill_attention: H must be a multiple of Hkv");
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8)
    throw std::runtime_error("prefill_attention: group size H/Hkv must be "
                             "1, 2, 4 or 8");
  if ((int64_t)T * G > (int64_t)1 << 30 ||
      (int64_t)B * T * Hkv > (int64_t)1 << 34)
    throw std::runtime_error("prefill_attention: T * G or B * T * Hkv too "
                             "large");
  if (!(scale > 0.f))
    throw std::runtime_error("prefill_attention: scale must be > 0");
  if (rope && !(rope_theta > 0.f))
    throw std::runtime_error("prefill_attention: rope_theta must be > 0");
  if (pos_stride != 0 && pos_stride != 1)
    throw std::runtime_error("prefill_attention: pos_stride must be 0 or 1");
  if ((k_new == nullptr) != (v_new == nullptr))
    throw std::runtime_error("prefill_attention: k_new/v_new go together");
  return G;
}

}  // namespace

void prefill_attention_mx(const void* q, const void* k_new, const void* v_new,
                          void* k_codes, void* v_codes, void* k_scales,
                          void* v_scales, const int64_t* pos, int pos_stride,
                          void* out, int B, int T, int H, int Hkv, int S_max,
                          int D, float scale, bool rope, float rope_theta,
                          int64_t q_bs, int64_t q_ts, int64_t q_hs,
                          int64_t n_bs, int64_t n_ts, int64_t n_hs,
                          int64_t c_bs, int64_t c_hs, int64_t c_rs,
                          int64_t s_bs, int64_t s_hs, int64_t s_rs,
                          hipStream_t stream) {
  const int G = check_problem(B, T, H, Hkv, S_max, D, scale, rope, rope_theta,
                              pos_stride, k_new, v_new);
  if (!q || !k_codes || !v_codes || !k_scales || !v_scales || !pos || !out)
    throw std::runtime_error("prefill_attention: null operand");
  if (!aligned16(q) || !aligned16(k_new) || !aligned16(v_new) ||
      !aligned16(out) || ((q_bs | q_ts | q_hs) & 7) ||
      (k_new && ((n_bs | n_ts | n_hs) & 7)))
    throw std::runtime_error(
        "prefill_attention: q, k_new, v_new and out must be 16-byte aligned "
        "with strides that are multiples of 8 elements");
  if ((reinterpret_cast<uintptr_t>(k_codes) & 7) ||
      (reinterpret_cast<uintptr_t>(v_codes) & 7) ||
      ((c_bs | c_hs | c_rs) & 7))
    throw std::runtime_error(
        "prefill_attention: MX cache code rows must be 8-byte aligned (base "
        "and strides multiples of 8 bytes)");
  if (c_rs < D || s_rs < D / 32)
    throw std::runtime_error("prefill_attention: MX cache row stride below "
                             "D codes or D / 32 scale bytes");

  const float ltheta = rope ? logf(rope_theta) : 0.f;
  const float neg2 = -2.0f / D;
  // the kernels' cache pointers are typed for the bf16 case; KV8 reads them
  // as bytes
  bf16_t* kcp = static_cast<bf16_t*>(k_codes);
  bf16_t* vcp = static_cast<bf16_t*>(v_codes);
  uint8_t* ksp = static_cast<uint8_t*>(k_scales);
  uint8_t* vsp = static_cast<uint8_t*>(v_scales);
  int lg = 0;
  while ((1 << lg) < G) ++lg;

#define PA8_LAUNCH(DD, RR)                                                   \
  do {                                                                       \
    if (k_new) {                                                             \
      const int64_t n = (int64_t)B * T * Hkv * (DD / 8);                     \
      hipLaunchKernelGGL((prefill_append_kernel<DD, RR, true>),              \
                         dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0,   \
                         stream, static_cast<const bf16_t*>(k_new),          \
                         static_cast<const bf16_t*>(v_new), kcp, vcp, pos,   \
                         pos_stride, B, T, Hkv, S_max, neg2, ltheta, n_bs,   \
                         n_ts, n_hs, c_bs, c_hs, c_rs, ksp, vsp, s_bs, s_hs, \
                         s_rs);                                              \
    }                                                                        \
    hipLaunchKernelGGL((prefill_attn_kernel<DD, RR, true>),                  \
                       dim3((T * G + QB - 1) / QB, Hkv, B), dim3(NT), 0,     \
                       stream, static_cast<const bf16_t*>(q), kcp, vcp, pos, \
                       pos_stride, static_cast<bf16_t*>(out), T, H, lg,      \
                       S_max, scale, neg2, ltheta, q_bs, q_ts, q_hs, c_bs,   \
                       c_hs, c_rs, ksp, vsp, s_bs, s_hs, s_rs);              \
  } while (0)
  if (D == 64) {
    if (rope) PA8_LAUNCH(64, true); else PA8_LAUNCH(64, false);
  } else {
    if (rope) PA8_LAUNCH(128, true); else PA8_LAUNCH(128, false);
  }
#undef PA8_LAUNCH
}

void prefill_attention_bf16(const void* q, const void* k_new,
                            const void* v_new, void* k_cache, void* v_cache,
                            const int64_t* pos, int pos_stride, void* out,
                            int B, int T, int H, int Hkv, int S_max, int D,
                            float scale, bool rope, float rope_theta,
                            int64_t q_bs, int64_t q_ts, int64_t q_hs,
                            int64_t n_bs, int64_t n_ts, int64_t n_hs,
                            int64_t c_bs, int64_t c_hs, int64_t c_rs,
                            hipStream_t stream) {
  const int G = check_problem(B, T, H, Hkv, S_max, D, scale, rope, rope_theta,
                              pos_stride, k_new, v_new);
  if (!q || !k_cache || !v_cache || !pos || !out)
    throw std::runtime_error("prefill_attention: null operand");
  // 16-byte vector access on every row: bases and strides in 8-element units
  if (!aligned16(q) || !aligned16(k_new) || !aligned16(v_new) ||
      !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out) ||
      ((q_bs | q_ts | q_hs | c_bs | c_hs | c_rs) & 7) ||
      (k_new && ((n_bs | n_ts | n_hs) & 7)))
    throw std::runtime_error(
        "prefill_attention: operands must be 16-byte aligned with strides "
        "that are multiples of 8 elements");
  if (c_rs < D)
    throw std::runtime_error("prefill_attention: cache row stride < D");

  const float ltheta = rope ? logf(rope_theta) : 0.f;
  const float neg2 = -2.0f / D;
  const bf16_t* qp = static_cast<const bf16_t*>(q);
  bf16_t* kcp = static_cast<bf16_t*>(k_cache);
  bf16_t* vcp = static_cast<bf16_t*>(v_cache);
  int lg = 0;
  while ((1 << lg) < G) ++lg;

#define PA_LAUNCH(DD, RR)                                                    \
  do {                                                                       \
    if (k_new) {                                                             \
      const int64_t n = (int64_t)B * T * Hkv * (DD / 8);                     \
      hipLaunchKernelGGL((prefill_append_kernel<DD, RR>),                    \
                         dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0,   \
                         stream, static_cast<const bf16_t*>(k_new),          \
                         static_cast<const bf16_t*>(v_new), kcp, vcp, pos,   \
                         pos_stride, B, T, Hkv, S_max, neg2, ltheta, n_bs,   \
                         n_ts, n_hs, c_bs, c_hs, c_rs, nullptr, nullptr,     \
                         (int64_t)0, (int64_t)0, (int64_t)0);                \
    }                                                                        \
    hipLaunchKernelGGL((prefill_attn_kernel<DD, RR>),                        \
                       dim3((T * G + QB - 1) / QB, Hkv, B), dim3(NT), 0,     \
                       stream, qp, kcp, vcp, pos, pos_stride,                \
                       static_cast<bf16_t*>(out), T, H, lg, S_max, scale,    \
                       neg2, ltheta, q_bs, q_ts, q_hs, c_bs, c_hs, c_rs,     \
                       nullptr, nullptr, (int64_t)0, (int64_t)0,             \
                       (int64_t)0);                                          \
  } while (0)
  if (D == 64) {
    if (rope) PA_LAUNCH(64, true); else PA_LAUNCH(64, false);
  } else {
    if (rope) PA_LAUNCH(128, true); else PA_LAUNCH(128, false);
  }
#undef PA_LAUNCH
}

}  // namespace tepdist
