// Single-query attention over an MXFP8 KV cache for gfx950: the grouped-query
// + RoPE decode kernel of decode_attention.hip reading e4m3 codes and e8m0
// block scales (ops/mx.py, MXCache) instead of bf16 rows. The cache is 51.6 %
// of the bf16 bytes; q, k_new, v_new and out stay bf16.
//
// What carries over unchanged from decode_attn_gqa_kernel: one 256-thread
// workgroup per (split, KV head, batch row) on a static grid; the position
// is read and clamped on the device; LPR = D / 8 lanes per row, 8 elements
// per lane; G query fragments and G online-softmax states (m, l, acc[8]) in
// fp32 registers on exp2; the wave, LDS and split merges; the fp32
// workspace (m, l, acc[D]) and its combine kernel (a copy: the bf16 file is
// left as it is); the finite "minus infinity".
//
// What is new:
//   - A lane's K (or V) fragment is one 8-byte load of 8 codes, half the
//     bytes of the bf16 kernel's load, so the ping-pong sets are deeper:
//     8 row groups for G <= 2 (the bf16 kernel's bytes in flight), 6 for
//     G = 4, 2 for G = 8, the deepest that keep two waves per SIMD.
//   - Scales: the four lanes (a quad) that share a 32-element block load
//     the block's byte once per row group and operand (a byte load from
//     the same address in the four lanes), form 2^(byte - 127) as
//     byte << 23 and hand it to v_cvt_scalef32_pk_f32_fp8, which converts
//     two codes and applies the scale in one instruction: half an
//     instruction per element where the bf16 unpack costs one. An e4m3
//     element times an in-range scale is exact in fp32, so the products
//     and sums see exactly the dequantized values.
//   - The new row: every lane rotates (ROPE) and rounds its 8 elements of
//     k_new to bf16 once, then quantizes them and its 8 elements of v_new by
//     the integer rule of mx_gemm_a8_plan.h (mxkv_quant8 of mx_kv.h: the
//     rule of mx.mx_quantize, no hardware saturating convert). The block
//     amax is the integer maximum of the magnitude bits over the quad, two
//     quad_perm DPP steps. The codes and the scale byte stay in registers
//     and are what the attend uses, through the same convert as a cache
//     row; the split == 0 workgroup stores the codes with one 8-byte store
//     per lane and the scale byte from the first lane of each quad.
//
// Position semantics are those of decode_attention.hip: with k_new the
// launch attends cache rows 0..p-1 plus the new row and never reads cache
// row p (lanes whose row is p load 8 in-bounds bytes of k_new instead and
// discard them); rows above p are never loaded, codes or scales: lanes past
// the split's end re-load its last valid row and are switched off by
// selects. All stores are vector stores; no atomics.

#include <cmath>
#include <stdexcept>

#include "common.h"
#include "kernels.h"
#include "mx_kv.h"
#include "rope_common.h"

namespace tepdist {

namespace {

constexpr int NT = 256;
constexpr int NW = NT / WAVE;
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

DEV_INLINE uint32_t pack2(float lo, float hi) {
  return (uint32_t)__builtin_bit_cast(unsigned short, f2bf(lo)) |
         ((uint32_t)__builtin_bit_cast(unsigned short, f2bf(hi)) << 16);
}

// U: row groups per register set (two sets in ping-pong).
template <int D, int G, bool ROPE, int U>
__launch_bounds__(NT) __global__
void decode_attn_mx_kernel(const bf16_t* __restrict__ q,
                           const bf16_t* __restrict__ k_new,
                           const bf16_t* __restrict__ v_new,
                           uint8_t* k_codes, uint8_t* v_codes,
                           uint8_t* k_scales, uint8_t* v_scales,
                           const int64_t* __restrict__ pos, int pos_stride,
                           bf16_t* __restrict__ out, float* __restrict__ ws,
                           int H, int S_max, float scale_log2e,
                           float neg2_over_d, float ltheta, int64_t q_bs,
                           int64_t q_hs, int64_t n_bs, int64_t n_hs,
                           int64_t c_bs, int64_t c_hs, int64_t c_rs,
                           int64_t s_bs, int64_t s_hs, int64_t s_rs) {
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

  const int64_t c_off = b * c_bs + hk * c_hs + col;
  const int64_t s_off = b * s_bs + hk * s_hs + (col >> 5);
  const uint8_t* kc = k_codes + c_off;
  const uint8_t* vc = v_codes + c_off;
  const uint8_t* ks = k_scales + s_off;
  const uint8_t* vs = v_scales + s_off;
  const bf16_t* kn = append ? k_new + b * n_bs + hk * n_hs : nullptr;
  const bf16_t* vn = append ? v_new + b * n_bs + hk * n_hs : nullptr;
  // what a lane whose row is the new one loads instead of cache row p:
  // 8 bytes and 1 byte of its own k_new fragment, in bounds, never used
  const uint8_t* dummy =
      append ? reinterpret_cast<const uint8_t*>(kn + col) : kc;

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

  // the new row as the cache will hold it: this lane's 8 codes of K and of
  // V and the two block scale bytes (6 VGPRs), kept for the attend
  unsigned kq0 = 0u, kq1 = 0u, kqb = 127u, vq0 = 0u, vq1 = 0u, vqb = 127u;
  if (append) {  // uniform: the DPP steps in mxkv_quant8 see every lane
    uint4 kv = *reinterpret_cast<const uint4*>(kn + col);
    const uint4 vv = *reinterpret_cast<const uint4*>(vn + col);
    if (ROPE) {
      float x[8], xp[8];
      unpack8(kv, x);
      unpack8(*reinterpret_cast<const uint4*>(kn + pcol), xp);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = x[e] * cs[e] + xp[e] * sn[e];
      kv = make_uint4(pack2(x[0], x[1]), pack2(x[2], x[3]),
                      pack2(x[4], x[5]), pack2(x[6], x[7]));
    }
    mxkv_quant8(kv.x, kv.y, kv.z, kv.w, kq0, kq1, kqb);
    mxkv_quant8(vv.x, vv.y, vv.z, vv.w, vq0, vq1, vqb);
    if (split == 0 && wid == 0 && lane < 2 * LPR) {
      // lanes [0, LPR) store K, [LPR, 2*LPR) store V: one 8-byte vector
      // store of codes each and one scale byte per quad, into cache row p
      // (a row nobody in this launch reads)
      const bool is_v = lane >= LPR;
      uint8_t* cb = is_v ? v_codes : k_codes;
      uint8_t* sb = is_v ? v_scales : k_scales;
      *reinterpret_cast<uint2*>(cb + c_off + (int64_t)p * c_rs) =
          is_v ? make_uint2(vq0, vq1) : make_uint2(kq0, kq1);
      if ((lane & 3) == 0)
        sb[s_off + (int64_t)p * s_rs] = (uint8_t)(is_v ? vqb : kqb);
    }
  }

  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = NEG;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  }

  // one register set: U row groups of K and V codes (2 VGPRs each) and
  // their scale bytes. Rows at or past r1 re-load the split's last valid
  // row, codes and scales alike.
  auto load = [&](int g0, uint2 (&kk)[U], uint2 (&vv)[U], unsigned (&kb)[U],
                  unsigned (&vb)[U]) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int r = r0 + (g0 + NW * j) * RPW + sub;
      const int rc = r < r1 ? r : r1 - 1;  // r1 > r0 >= 0 when called
      const bool nw = rc == p_new;
      kk[j] = *reinterpret_cast<const uint2*>(
          nw ? dummy : kc + (int64_t)rc * c_rs);
      vv[j] = *reinterpret_cast<const uint2*>(
          nw ? dummy : vc + (int64_t)rc * c_rs);
      kb[j] = *(nw ? dummy : ks + (int64_t)rc * s_rs);
      vb[j] = *(nw ? dummy : vs + (int64_t)rc * s_rs);
    }
  };
  auto consume = [&](int g0, const uint2 (&kk)[U], const uint2 (&vv)[U],
                     const unsigned (&kb)[U], const unsigned (&vb)[U]) {
    float s[G][U];
    bool ok[U], nw[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int r = r0 + (g0 + NW * j) * RPW + sub;
      ok[j] = r < r1;
      // the new row is attended from registers; a switched-off lane whose
      // clamped row is the new one takes it too, so its values are finite
      nw[j] = (ok[j] ? r : r1 - 1) == p_new;
      float kf[8];
      mxkv_dq8(nw[j] ? kq0 : kk[j].x, nw[j] ? kq1 : kk[j].y,
          nw[j] ? kqb : kb[j], kf);
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
      mxkv_dq8(nw[j] ? vq0 : vv[j].x, nw[j] ? vq1 : vv[j].y,
          nw[j] ? vqb : vb[j], vf);
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
  // look-ahead load, as in decode_attention.hip
  constexpr int STEP = NW * U;
  if (ng > 0) {
    uint2 ka[U], va[U], kb[U], vb[U];
    unsigned ksa[U], vsa[U], ksb[U], vsb[U];
    int g0 = wid;
    load(g0, ka, va, ksa, vsa);
    while (g0 < ng) {
      load(g0 + STEP, kb, vb, ksb, vsb);
      consume(g0, ka, va, ksa, vsa);
      g0 += STEP;
      if (g0 >= ng) break;
      load(g0 + STEP, ka, va, ksa, vsa);
      consume(g0, kb, vb, ksb, vsb);
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

// log-sum-exp combine of the per-split partials; one block of D threads
// per (b, h). The workspace layout and this kernel are those of
// decode_attention.hip.
template <int D>
__launch_bounds__(D) __global__
void decode_attn_mx_combine_kernel(const float* __restrict__ ws,
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

bool aligned(const void* p, int n) {
  return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0;
}

}  // namespace

void decode_attention_mx(const void* q, const void* k_new, const void* v_new,
                         void* k_codes, void* v_codes, void* k_scales,
                         void* v_scales, const int64_t* pos, int pos_stride,
                         void* out, float* ws, int B, int H, int Hkv,
                         int S_max, int D, float scale, int splits, bool rope,
                         float rope_theta, int64_t q_bs, int64_t q_hs,
                         int64_t n_bs, int64_t n_hs, int64_t c_bs,
                         int64_t c_hs, int64_t c_rs, int64_t s_bs,
                         int64_t s_hs, int64_t s_rs, hipStream_t stream) {
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
  if (!q || !k_codes || !v_codes || !k_scales || !v_scales || !pos || !out ||
      (splits > 1 && !ws))
    throw std::runtime_error("decode_attention: null operand");
  // 16-byte vector access on every bf16 row, 8-byte on every code row
  if (!aligned(q, 16) || !aligned(k_new, 16) || !aligned(v_new, 16) ||
      ((q_bs | q_hs) & 7) || (k_new && ((n_bs | n_hs) & 7)))
    throw std::runtime_error(
        "decode_attention: q, k_new and v_new must be 16-byte aligned with "
        "strides that are multiples of 8 elements");
  if (!aligned(k_codes, 8) || !aligned(v_codes, 8) ||
      ((c_bs | c_hs | c_rs) & 7))
    throw std::runtime_error(
        "decode_attention: MX cache code rows must be 8-byte aligned (base "
        "and strides multiples of 8 bytes)");
  if (c_rs < D || s_rs < D / 32)
    throw std::runtime_error("decode_attention: MX cache row stride below "
                             "D codes or D / 32 scale bytes");

  const dim3 grid(splits, Hkv, B), blk(NT);
  const float sl = scale * LOG2E;
  const float ltheta = rope ? logf(rope_theta) : 0.f;
  const float neg2 = -2.0f / D;
  const bf16_t* qp = static_cast<const bf16_t*>(q);
  const bf16_t* knp = static_cast<const bf16_t*>(k_new);
  const bf16_t* vnp = static_cast<const bf16_t*>(v_new);
  bf16_t* op = static_cast<bf16_t*>(out);
  // set depth: 8 row groups for G <= 2. G = 4 takes 6 and G = 8 takes 2: with
  // the G x U scores and a scale register per row group and operand, 8 and 4
  // compile to 256 VGPRs plus AGPR copies, one wave per SIMD; 6 and 2 keep
  // the bf16 kernel's two (docs/KERNELS.md "MXFP8 KV cache")
#define DM_LAUNCH(DD, GG, RR)                                               \
  do {                                                                      \
    hipLaunchKernelGGL(                                                     \
        (decode_attn_mx_kernel<DD, GG, RR, (GG == 8 ? 2 : GG == 4 ? 6 : 8)>),  \
        grid, blk,                                                          \
        0, stream, qp, knp, vnp, static_cast<uint8_t*>(k_codes),            \
        static_cast<uint8_t*>(v_codes), static_cast<uint8_t*>(k_scales),    \
        static_cast<uint8_t*>(v_scales), pos, pos_stride, op, ws, H, S_max, \
        sl, neg2, ltheta, q_bs, q_hs, n_bs, n_hs, c_bs, c_hs, c_rs, s_bs,   \
        s_hs, s_rs);                                                        \
    if (splits > 1)                                                         \
      hipLaunchKernelGGL(decode_attn_mx_combine_kernel<DD>, dim3(B * H),    \
                         dim3(DD), 0, stream, ws, op, splits);              \
  } while (0)
#define DM_ROPE(DD, GG)                                                     \
  do {                                                                      \
    if (rope) DM_LAUNCH(DD, GG, true); else DM_LAUNCH(DD, GG, false);       \
  } while (0)
#define DM_GROUP(DD)                                                        \
  do {                                                                      \
    switch (G) {                                                            \
      case 1: DM_ROPE(DD, 1); break;                                        \
      case 2: DM_ROPE(DD, 2); break;                                        \
      case 4: DM_ROPE(DD, 4); break;                                        \
      default: DM_ROPE(DD, 8); break;                                       \
    }                                                                       \
  } while (0)
  if (D == 64) DM_GROUP(64); else DM_GROUP(128);
#undef DM_GROUP
#undef DM_ROPE
#undef DM_LAUNCH
}

}  // namespace tepdist
