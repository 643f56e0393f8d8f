// Single-query ("flash-decoding") attention over a KV cache for gfx950.
//
// One 256-thread workgroup per (split, head, batch row). The valid length
// is read on the device from `pos`, so a captured launch stays valid while
// the position advances; the grid (splits, H, B) never changes.
//
// Lane mapping: a K/V row is D bf16 = D/8 lanes x 16 B, so one
// global_load_dwordx4 of a wave covers 64/(D/8) whole rows, fully
// coalesced (D=64: 8 rows, D=128: 4 rows). K and V go straight to VGPRs,
// UNROLL row groups in flight before the first use; nothing streamed
// passes through LDS. Each group of D/8 lanes keeps its own online-softmax
// state (m, l, acc[8]) in fp32 on exp2 (scale * log2e folded into q); the
// states are merged across the wave by __shfl_xor, across the 4 waves by a
// small LDS area, and across splits by a second small kernel.
//
// Position semantics (p = clamp(pos[b], 0, S_max-1) — an out-of-range
// position is clamped, so no load or store can leave the cache):
//   k_new == null : attend cache rows 0..p.
//   k_new != null : attend cache rows 0..p-1 plus the new row, which is
//                   taken from k_new/v_new, never from the cache. The
//                   workgroup with split == 0 also stores the new row into
//                   cache[b, h, p, :]. No workgroup of the launch reads
//                   that cache row, so there is no cross-workgroup hazard.
// Rows above p are never loaded: out-of-range lanes re-load the last valid
// row of their split and are switched off by selects on the score and on
// the probability, so whatever those rows hold (NaN, Inf) has no effect.
//
// Grouped-query attention + RoPE (decode_attn_gqa_kernel): caches hold Hkv
// heads, q holds H = G * Hkv; query head h attends K/V head h / G. One
// workgroup per (split, KV head, batch row) keeps the G query fragments and
// G online-softmax states in registers, so each K/V row is loaded once and
// used G times. With ROPE, q and k_new are rotated in fp32 at the same
// clamped p that indexes the cache (angles from rope_common.h, shared with
// the prefill rope_kernel): q stays fp32; k_new is rounded to bf16 once and
// that value is both attended to and stored, so the cache holds rotated
// rows. The G == 1, no-rope call keeps the original decode_attn_kernel.

#include <cmath>
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "rope_common.h"

namespace tepdist {

namespace {

constexpr int NT = 256;
constexpr int NW = NT / WAVE;
constexpr int UNROLL = 4;
constexpr float NEG = -3.0e38f;  // finite "minus infinity": NEG - NEG == 0
constexpr float LOG2E = 1.4426950408889634f;

DEV_INLINE void unpack8(const uint4& u, float* f) {
  f[0] = __uint_as_float(u.x << 16);
  f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = __uint_as_float(u.y << 16);
  f[3] = __uint_as_float(u.y & 0xffff0000u);
  f[4] = __uint_as_float(u.z << 16);
  f[5] = __uint_as_float(u.z & 0xffff0000u);
  f[6] = __uint_as_float(u.w << 16);
  f[7] = __uint_as_float(u.w & 0xffff0000u);
}

DEV_INLINE float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

template <int D>
__launch_bounds__(NT) __global__
void decode_attn_kernel(const bf16_t* __restrict__ q,
                        const bf16_t* __restrict__ k_new,
                        const bf16_t* __restrict__ v_new,
                        bf16_t* k_cache, bf16_t* v_cache,
                        const int64_t* __restrict__ pos, int pos_stride,
                        bf16_t* __restrict__ out, float* __restrict__ ws,
                        int H, int S_max, float scale_log2e, int64_t q_bs,
                        int64_t q_hs, int64_t n_bs, int64_t n_hs,
                        int64_t c_bs, int64_t c_hs, int64_t c_rs) {
  constexpr int LPR = D / 8;       // lanes per row
  constexpr int RPW = WAVE / LPR;  // rows per wave-wide load
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int sub = lane / LPR;
  const int col = (lane % LPR) * 8;

  int64_t p64 = pos[(int64_t)b * pos_stride];
  p64 = p64 < 0 ? 0 : p64;
  p64 = p64 > S_max - 1 ? S_max - 1 : p64;
  const int p = (int)p64;
  const bool append = k_new != nullptr;
  const int p_new = append ? p : -1;  // logical row served by k_new/v_new
  const int n_tot = p + 1;

  // balanced split of the valid rows, computed from the device position
  int L = (n_tot + nsplit - 1) / nsplit;
  L = (L + RPW - 1) / RPW * RPW;
  const int r0 = min(split * L, n_tot);
  const int r1 = min(r0 + L, n_tot);
  const int ng = (r1 - r0 + RPW - 1) / RPW;  // row groups of this split

  const bf16_t* kc = k_cache + b * c_bs + h * c_hs + col;
  const bf16_t* vc = v_cache + b * c_bs + h * c_hs + col;
  const bf16_t* kn = append ? k_new + b * n_bs + h * n_hs + col : nullptr;
  const bf16_t* vn = append ? v_new + b * n_bs + h * n_hs + col : nullptr;

  if (append && split == 0 && wid == 0 && lane < 2 * LPR) {
    // lanes [0, LPR) store K, [LPR, 2*LPR) store V: one 16-B vector
    // store each into cache row p (a row nobody in this launch reads)
    const bool is_v = lane >= LPR;
    bf16_t* base = is_v ? v_cache : k_cache;
    const bf16_t* src = is_v ? vn : kn;
    *reinterpret_cast<uint4*>(base + b * c_bs + h * c_hs +
                              (int64_t)p * c_rs + col) =
        *reinterpret_cast<const uint4*>(src);
  }

  float qf[8];
  {
    const uint4 qv =
        *reinterpret_cast<const uint4*>(q + b * q_bs + h * q_hs + col);
    unpack8(qv, qf);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[e] *= scale_log2e;
  }

  float m = NEG, l = 0.f;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;

  // UNROLL row groups (K and V: 2*UNROLL dwordx4 loads per lane) issued
  // back to back; rows at or past r1 re-load the split's last valid row.
  auto load = [&](int g0, uint4 (&kk)[UNROLL], uint4 (&vv)[UNROLL]) {
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      const int r = r0 + (g0 + NW * j) * RPW + sub;
      const int rc = r < r1 ? r : r1 - 1;  // r1 > r0 >= 0 when called
      const bool nw = rc == p_new;
      const bf16_t* kp = nw ? kn : kc + (int64_t)rc * c_rs;
      const bf16_t* vp = nw ? vn : vc + (int64_t)rc * c_rs;
      kk[j] = *reinterpret_cast<const uint4*>(kp);
      vv[j] = *reinterpret_cast<const uint4*>(vp);
    }
  };
  auto consume = [&](int g0, const uint4 (&kk)[UNROLL],
                     const uint4 (&vv)[UNROLL]) {
    float s[UNROLL];
    bool ok[UNROLL];
    float m_new = m;
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      ok[j] = r0 + (g0 + NW * j) * RPW + sub < r1;
      float kf[8];
      unpack8(kk[j], kf);
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) dot += qf[e] * kf[e];
#pragma unroll
      for (int off = LPR / 2; off > 0; off >>= 1)
        dot += __shfl_xor(dot, off, 64);
      s[j] = ok[j] ? dot : NEG;
      m_new = fmaxf(m_new, s[j]);
    }
    const float alpha = ex2(m - m_new);
    l *= alpha;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      const float pj = ok[j] ? ex2(s[j] - m_new) : 0.f;
      float vf[8];
      unpack8(vv[j], vf);
      l += pj;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += pj * vf[e];
    }
    m = m_new;
  };

  // two register sets in ping-pong: the next set's loads are issued before
  // the current set is consumed, so a wave always has loads in flight. The
  // look-ahead load is unconditional (past the end it re-reads the last
  // valid row): a branch around it would make the compiler's vmcnt at the
  // join wait for the look-ahead set as well.
  constexpr int STEP = NW * UNROLL;
  if (ng > 0) {
    uint4 ka[UNROLL], va[UNROLL], kb[UNROLL], vb[UNROLL];
    int g0 = wid;
    load(g0, ka, va);
    while (g0 < ng) {
      load(g0 + STEP, kb, vb);
      consume(g0, ka, va);
      g0 += STEP;
      if (g0 >= ng) break;
      load(g0 + STEP, ka, va);
      consume(g0, kb, vb);
      g0 += STEP;
    }
  }

  // merge the RPW lane groups of the wave
#pragma unroll
  for (int off = LPR; off < WAVE; off <<= 1) {
    const float m_o = __shfl_xor(m, off, 64);
    const float l_o = __shfl_xor(l, off, 64);
    const float mm = fmaxf(m, m_o);
    const float a = ex2(m - mm), c = ex2(m_o - mm);
    l = l * a + l_o * c;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      acc[e] = acc[e] * a + __shfl_xor(acc[e], off, 64) * c;
    m = mm;
  }

  // merge the block's waves through LDS
  __shared__ float sm_m[NW], sm_l[NW], sm_acc[NW][D];
  if (lane < LPR) {
#pragma unroll
    for (int e = 0; e < 8; ++e) sm_acc[wid][col + e] = acc[e];
    if (lane == 0) {
      sm_m[wid] = m;
      sm_l[wid] = l;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < D) {
    float mm = sm_m[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) mm = fmaxf(mm, sm_m[w]);
    float lt = 0.f, at = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float c = ex2(sm_m[w] - mm);
      lt += c * sm_l[w];
      at += c * sm_acc[w][t];
    }
    const int64_t bh = (int64_t)b * H + h;
    if (nsplit == 1) {
      // split 0 always holds row 0, so lt > 0
      out[bh * D + t] = f2bf(at / lt);
    } else {
      // an empty split writes (NEG, 0, 0...) and weighs exactly 0 below
      float* w = ws + (bh * nsplit + split) * (D + 2);
      if (t == 0) {
        w[0] = mm;
        w[1] = lt;
      }
      w[2 + t] = at;
    }
  }
}

DEV_INLINE uint32_t pack2(float lo, float hi) {
  return (uint32_t)__builtin_bit_cast(unsigned short, f2bf(lo)) |
         ((uint32_t)__builtin_bit_cast(unsigned short, f2bf(hi)) << 16);
}

// GQA (+ optional RoPE) variant: same streaming loop, G queries per K/V
// row. U is the row-group unroll (UNROLL, or less where G queries' state
// would push the kernel past 256 VGPRs).
template <int D, int G, bool ROPE, int U>
__launch_bounds__(NT) __global__
void decode_attn_gqa_kernel(const bf16_t* __restrict__ q,
                            const bf16_t* __restrict__ k_new,
                            const bf16_t* __restrict__ v_new,
                            bf16_t* k_cache, bf16_t* v_cache,
                            const int64_t* __restrict__ pos, int pos_stride,
                            bf16_t* __restrict__ out, float* __restrict__ ws,
                            int H, int S_max, float scale_log2e,
                            float neg2_over_d, float ltheta, int64_t q_bs,
                            int64_t q_hs, int64_t n_bs, int64_t n_hs,
                            int64_t c_bs, int64_t c_hs, int64_t c_rs) {
  constexpr int LPR = D / 8;       // lanes per row
  constexpr int RPW = WAVE / LPR;  // rows per wave-wide load
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int hk = blockIdx.y, b = blockIdx.z;  // hk: K/V head
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int sub = lane / LPR;
  const int col = (lane % LPR) * 8;
  const int pcol = col ^ (D / 2);  // RoPE partner elements (i +- D/2)

  int64_t p64 = pos[(int64_t)b * pos_stride];
  p64 = p64 < 0 ? 0 : p64;
  p64 = p64 > S_max - 1 ? S_max - 1 : p64;
  const int p = (int)p64;
  const bool append = k_new != nullptr;
  const int p_new = append ? p : -1;  // logical row served by k_new/v_new
  const int n_tot = p + 1;

  int L = (n_tot + nsplit - 1) / nsplit;
  L = (L + RPW - 1) / RPW * RPW;
  const int r0 = min(split * L, n_tot);
  const int r1 = min(r0 + L, n_tot);
  const int ng = (r1 - r0 + RPW - 1) / RPW;

  const bf16_t* kc = k_cache + b * c_bs + hk * c_hs + col;
  const bf16_t* vc = v_cache + b * c_bs + hk * c_hs + col;
  const bf16_t* kn = append ? k_new + b * n_bs + hk * n_hs : nullptr;
  const bf16_t* vn = append ? v_new + b * n_bs + hk * n_hs : nullptr;

  // rotation of this lane's 8 elements: y = x * cs + partner * sn, with
  // sn negated in the first half of the row (rotate-half)
  float cs[8], sn[8];
  if (ROPE) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s, c;
      rope_sincos(p, (col + e) & (D / 2 - 1), neg2_over_d, ltheta, &s, &c);
      cs[e] = c;
      sn[e] = col < D / 2 ? -s : s;
    }
  }

  // G query fragments, fp32, rotated (never rounded), scale*log2e folded in
  float qf[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const bf16_t* qp = q + b * q_bs + (int64_t)(hk * G + g) * q_hs;
    unpack8(*reinterpret_cast<const uint4*>(qp + col), qf[g]);
    if (ROPE) {
      float xp[8];
      unpack8(*reinterpret_cast<const uint4*>(qp + pcol), xp);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[g][e] = qf[g][e] * cs[e] + xp[e] * sn[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[g][e] *= scale_log2e;
  }

  // the new K row, rotated and rounded to bf16 once: every lane keeps its
  // own 8 elements (4 VGPRs) for the attend, lanes [0, LPR) store them
  // (four scalars, not a uint4: the struct would live in scratch)
  uint32_t kr0 = 0u, kr1 = 0u, kr2 = 0u, kr3 = 0u;
  if (ROPE && append) {
    float x[8], xp[8];
    unpack8(*reinterpret_cast<const uint4*>(kn + col), x);
    unpack8(*reinterpret_cast<const uint4*>(kn + pcol), xp);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = x[e] * cs[e] + xp[e] * sn[e];
    kr0 = pack2(x[0], x[1]);
    kr1 = pack2(x[2], x[3]);
    kr2 = pack2(x[4], x[5]);
    kr3 = pack2(x[6], x[7]);
  }

  if (append && split == 0 && wid == 0 && lane < 2 * LPR) {
    // lanes [0, LPR) store K, [LPR, 2*LPR) store V: one 16-B vector
    // store each into cache row p (a row nobody in this launch reads)
    const bool is_v = lane >= LPR;
    bf16_t* base = is_v ? v_cache : k_cache;
    uint4 val = *reinterpret_cast<const uint4*>((is_v ? vn : kn) + col);
    if (ROPE && !is_v) val = make_uint4(kr0, kr1, kr2, kr3);
    *reinterpret_cast<uint4*>(base + b * c_bs + hk * c_hs +
                              (int64_t)p * c_rs + col) = val;
  }

  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = NEG;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  }

  auto load = [&](int g0, uint4 (&kk)[U], uint4 (&vv)[U]) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int r = r0 + (g0 + NW * j) * RPW + sub;
      const int rc = r < r1 ? r : r1 - 1;  // r1 > r0 >= 0 when called
      const bool nw = rc == p_new;
      const bf16_t* kp = nw ? kn + col : kc + (int64_t)rc * c_rs;
      const bf16_t* vp = nw ? vn + col : vc + (int64_t)rc * c_rs;
      kk[j] = *reinterpret_cast<const uint4*>(kp);
      vv[j] = *reinterpret_cast<const uint4*>(vp);
    }
  };
  auto consume = [&](int g0, const uint4 (&kk)[U], const uint4 (&vv)[U]) {
    float s[G][U];
    bool ok[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int r = r0 + (g0 + NW * j) * RPW + sub;
      ok[j] = r < r1;
      uint4 ku = kk[j];
      if (ROPE) {  // the new row is attended in its rotated form
        const bool nw = r == p_new;
        ku.x = nw ? kr0 : ku.x;
        ku.y = nw ? kr1 : ku.y;
        ku.z = nw ? kr2 : ku.z;
        ku.w = nw ? kr3 : ku.w;
      }
      float kf[8];
      unpack8(ku, kf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) dot += qf[g][e] * kf[e];
#pragma unroll
        for (int off = LPR / 2; off > 0; off >>= 1)
          dot += __shfl_xor(dot, off, 64);
        s[g][j] = ok[j] ? dot : NEG;
      }
    }
    float m_new[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      m_new[g] = m[g];
#pragma unroll
      for (int j = 0; j < U; ++j) m_new[g] = fmaxf(m_new[g], s[g][j]);
      const float alpha = ex2(m[g] - m_new[g]);
      l[g] *= alpha;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] *= alpha;
      m[g] = m_new[g];
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      float vf[8];
      unpack8(vv[j], vf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pj = ok[j] ? ex2(s[g][j] - m_new[g]) : 0.f;
        l[g] += pj;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] += pj * vf[e];
      }
    }
  };

  // ping-pong over two register sets with an unconditional clamped
  // look-ahead load, as in decode_attn_kernel
  constexpr int STEP = NW * U;
  if (ng > 0) {
    uint4 ka[U], va[U], kb[U], vb[U];
    int g0 = wid;
    load(g0, ka, va);
    while (g0 < ng) {
      load(g0 + STEP, kb, vb);
      consume(g0, ka, va);
      g0 += STEP;
      if (g0 >= ng) break;
      load(g0 + STEP, ka, va);
      consume(g0, kb, vb);
      g0 += STEP;
    }
  }

  // merge the RPW lane groups of the wave, per group member
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int off = LPR; off < WAVE; off <<= 1) {
      const float m_o = __shfl_xor(m[g], off, 64);
      const float l_o = __shfl_xor(l[g], off, 64);
      const float mm = fmaxf(m[g], m_o);
      const float a = ex2(m[g] - mm), c = ex2(m_o - mm);
      l[g] = l[g] * a + l_o * c;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        acc[g][e] = acc[g][e] * a + __shfl_xor(acc[g][e], off, 64) * c;
      m[g] = mm;
    }
  }

  // merge the block's waves through LDS
  __shared__ float sm_m[G][NW], sm_l[G][NW], sm_acc[G][NW][D];
  if (lane < LPR) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm_acc[g][wid][col + e] = acc[g][e];
      if (lane == 0) {
        sm_m[g][wid] = m[g];
        sm_l[g][wid] = l[g];
      }
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < G * D; idx += NT) {
    const int g = idx / D, t = idx % D;
    float mm = sm_m[g][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) mm = fmaxf(mm, sm_m[g][w]);
    float lt = 0.f, at = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float c = ex2(sm_m[g][w] - mm);
      lt += c * sm_l[g][w];
      at += c * sm_acc[g][w][t];
    }
    const int64_t bh = (int64_t)b * H + hk * G + g;  // query head
    if (nsplit == 1) {
      out[bh * D + t] = f2bf(at / lt);
    } else {
      float* w = ws + (bh * nsplit + split) * (D + 2);
      if (t == 0) {
        w[0] = mm;
        w[1] = lt;
      }
      w[2 + t] = at;
    }
  }
}

// log-sum-exp combine of the per-split partials; one block of D threads
// per (b, h).
template <int D>
__launch_bounds__(D) __global__
void decode_attn_combine_kernel(const float* __restrict__ ws,
                                bf16_t* __restrict__ out, int nsplit) {
  const int64_t bh = blockIdx.x;
  const int t = threadIdx.x;
  const float* w = ws + bh * nsplit * (D + 2);
  float mm = NEG;
  for (int i = 0; i < nsplit; ++i) mm = fmaxf(mm, w[i * (D + 2)]);
  float lt = 0.f, at = 0.f;
  for (int i = 0; i < nsplit; ++i) {
    const float c = ex2(w[i * (D + 2)] - mm);
    lt += c * w[i * (D + 2) + 1];
    at += c * w[i * (D + 2) + 2 + t];
  }
  out[bh * D + t] = f2bf(at / lt);
}

bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace

void decode_attention_bf16(const void* q, const void* k_new,
                           const void* v_new, void* k_cache, void* v_cache,
                           const int64_t* pos, int pos_stride, void* out,
                           float* ws, int B, int H, int Hkv, int S_max,
                           int D, float scale, int splits, bool rope,
                           float rope_theta, int64_t q_bs,
                           int64_t q_hs, int64_t n_bs, int64_t n_hs,
                           int64_t c_bs, int64_t c_hs, int64_t c_rs,
                           hipStream_t stream) {
  if (D != 64 && D != 128)
    throw std::runtime_error("decode_attention: head dim must be 64 or 128");
  if (splits < 1 || splits > 32)
    throw std::runtime_error("decode_attention: splits must be in [1, 32]");
  if (B < 1 || B > 65535 || H < 1 || H > 65535 || S_max < 1)
    throw std::runtime_error("decode_attention: bad B/H/S_max");
  if (Hkv < 1 || H % Hkv != 0)
    throw std::runtime_error("decode_attention: H must be a multiple of Hkv");
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8)
    throw std::runtime_error("decode_attention: group size H/Hkv must be "
                             "1, 2, 4 or 8");
  if (rope && !(rope_theta > 0.f))
    throw std::runtime_error("decode_attention: rope_theta must be > 0");
  if (pos_stride != 0 && pos_stride != 1)
    throw std::runtime_error("decode_attention: pos_stride must be 0 or 1");
  if ((k_new == nullptr) != (v_new == nullptr))
    throw std::runtime_error("decode_attention: k_new/v_new go together");
  if (!q || !k_cache || !v_cache || !pos || !out || (splits > 1 && !ws))
    throw std::runtime_error("decode_attention: null operand");
  // 16-byte vector access on every row: bases and strides in 8-element units
  if (!aligned16(q) || !aligned16(k_new) || !aligned16(v_new) ||
      !aligned16(k_cache) || !aligned16(v_cache) ||
      ((q_bs | q_hs | c_bs | c_hs | c_rs) & 7) ||
      (k_new && ((n_bs | n_hs) & 7)))
    throw std::runtime_error(
        "decode_attention: operands must be 16-byte aligned with strides "
        "that are multiples of 8 elements");
  if (c_rs < D)
    throw std::runtime_error("decode_attention: cache row stride < D");

  const dim3 grid(splits, Hkv, B), blk(NT);
  const float sl = scale * LOG2E;
  const bf16_t* qp = static_cast<const bf16_t*>(q);
  const bf16_t* knp = static_cast<const bf16_t*>(k_new);
  const bf16_t* vnp = static_cast<const bf16_t*>(v_new);
  bf16_t* kcp = static_cast<bf16_t*>(k_cache);
  bf16_t* vcp = static_cast<bf16_t*>(v_cache);
  bf16_t* op = static_cast<bf16_t*>(out);
#define DA_LAUNCH(DD)                                                       \
  do {                                                                      \
    hipLaunchKernelGGL(decode_attn_kernel<DD>, grid, blk, 0, stream, qp,    \
                       knp, vnp, kcp, vcp, pos, pos_stride, op, ws, H,      \
                       S_max, sl, q_bs, q_hs, n_bs, n_hs, c_bs, c_hs,       \
                       c_rs);                                               \
    if (splits > 1)                                                         \
      hipLaunchKernelGGL(decode_attn_combine_kernel<DD>, dim3(B * H),       \
                         dim3(DD), 0, stream, ws, op, splits);              \
  } while (0)
  if (G == 1 && !rope) {
    if (D == 64) DA_LAUNCH(64); else DA_LAUNCH(128);
    return;
  }
#undef DA_LAUNCH
  const float ltheta = rope ? logf(rope_theta) : 0.f;
  const float neg2 = -2.0f / D;
  // G = 8 halves the unroll: 8 queries' state plus two 4-deep load sets
  // would not fit 256 VGPRs (two waves per SIMD)
#define DG_LAUNCH(DD, GG, RR)                                               \
  do {                                                                      \
    hipLaunchKernelGGL(                                                     \
        (decode_attn_gqa_kernel<DD, GG, RR, (GG == 8 ? UNROLL / 2 : UNROLL)>), \
        grid, blk, 0, stream, qp, knp, vnp, kcp, vcp, pos, pos_stride, op,  \
        ws, H, S_max, sl, neg2, ltheta, q_bs, q_hs, n_bs, n_hs, c_bs, c_hs, \
        c_rs);                                                              \
    if (splits > 1)                                                         \
      hipLaunchKernelGGL(decode_attn_combine_kernel<DD>, dim3(B * H),       \
                         dim3(DD), 0, stream, ws, op, splits);              \
  } while (0)
#define DG_ROPE(DD, GG)                                                     \
  do {                                                                      \
    if (rope) DG_LAUNCH(DD, GG, true); else DG_LAUNCH(DD, GG, false);       \
  } while (0)
#define DG_GROUP(DD)                                                        \
  do {                                                                      \
    switch (G) {                                                            \
      case 1: DG_LAUNCH(DD, 1, true); break; /* G == 1 gets here with rope */ \
      case 2: DG_ROPE(DD, 2); break;                                        \
      case 4: DG_ROPE(DD, 4); break;                                        \
      default: DG_ROPE(DD, 8); break;                                       \
    }                                                                       \
  } while (0)
  if (D == 64) DG_GROUP(64); else DG_GROUP(128);
#undef DG_GROUP
#undef DG_ROPE
#undef DG_LAUNCH
}

}  // namespace tepdist
