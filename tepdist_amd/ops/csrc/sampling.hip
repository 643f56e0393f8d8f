// Token sampling on the device: temperature, top-k and top-p over one row of
// logits per workgroup, drawn by inverse CDF from a Philox word (or a given
// uniform). Semantics: ops/reference.py sample_logits; design and measured
// numbers: docs/KERNELS.md "Sampling".
//
// Every weight is turned into a 2^-40 fixed-point integer once
// (q = trunc(w * 2^40), w = exp2((z - m) * log2e / T) in fp32) and all sums
// are 64-bit integer sums: histograms are LDS integer atomics, prefix sums
// are integer scans. Integer addition is associative, so every sum is exact
// and independent of the order the hardware performs it in: thresholds and
// tokens repeat bit for bit, running sums are monotone, and the row total
// equals the last running sum.
//
// Both thresholds are exact k-th-value selections by a 4 x 8-bit radix
// descent over the order-preserving 32-bit key of z: top-k descends on
// counts, top-p on the fixed-point weights of what top-k left.

#include "common.h"
#include "kernels.h"

#include <climits>
#include <cmath>

namespace tepdist {
namespace {

constexpr int ST = 1024;                   // threads per row
constexpr int SW = ST / WAVE;              // waves per row
constexpr int RC = 16;                     // histogram copies (lane & 15)
constexpr float kFix = 1099511627776.0f;   // 2^40

typedef unsigned long long u64;

// Order-preserving key: a < b as floats <=> key(a) < key(b) as unsigned
// (-0 folded onto +0; NaNs land above +inf or below -inf by their sign).
DEV_INLINE uint32_t key_of(float z) {
  uint32_t b = __float_as_uint(z);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

DEV_INLINE float val_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// q = trunc(w * 2^40) with w = exp2((z - m) * c), exactly 2^40 at z == m
// (also when m is +-inf) and 0 for -inf, NaN and anything out of [0, 1].
DEV_INLINE u64 weight_q(float z, float m, float c) {
  float w = __builtin_amdgcn_exp2f((z - m) * c);
  if (z == m) w = 1.0f;
  w = (w >= 0.0f) ? fminf(w, 1.0f) : 0.0f;
  return static_cast<u64>(w * kFix);
}

// ceil(f * W) clamped to [1, W]: the running sum that has to be reached.
DEV_INLINE u64 frac_target(float f, u64 W) {
  const double t = ceil(static_cast<double>(f) * static_cast<double>(W));
  u64 q = (t >= 9.0e18) ? W : static_cast<u64>(t);
  q = q < W ? q : W;
  return q > 1 ? q : 1;
}

// A row read in 16-byte groups. base = row start rounded down to 16 bytes
// (`a` elements earlier), so group g covers shifted indices g*VEC .. +VEC-1
// and column i = g*VEC + e - a. Groups wholly inside [0, vocab) take one
// 16-byte load; the (at most two) edge groups of a row whose start or end
// is not 16-byte aligned take element loads of their valid columns only, so
// nothing outside the row's columns [0, vocab) is ever read.
template <typename T>
struct Row {
  static constexpr int VEC = 16 / sizeof(T);
  const T* base;
  int a, vocab, ngroups;

  DEV_INLINE Row(const T* row, int vocab_) : vocab(vocab_) {
    a = static_cast<int>((reinterpret_cast<uintptr_t>(row) & 15) / sizeof(T));
    base = row - a;
    ngroups = (a + vocab + VEC - 1) / VEC;
  }

  DEV_INLINE static float cvt(float v) { return v; }
  DEV_INLINE static float cvt(uint16_t v) {
    return __uint_as_float(static_cast<uint32_t>(v) << 16);
  }

  // z[e] and bit e of the result for every valid column of group g
  DEV_INLINE unsigned load(int g, float (&z)[VEC]) const {
    const int i0 = g * VEC - a;
    if (i0 >= 0 && i0 + VEC <= vocab) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(base + g * VEC);
      if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) z[e] = __uint_as_float(v[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          z[2 * e] = __uint_as_float(v[e] << 16);
          z[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
        }
      }
      return (1u << VEC) - 1u;
    }
    unsigned mask = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int i = i0 + e;
      z[e] = 0.0f;
      if (i >= 0 && i < vocab) {
        z[e] = cvt(base[g * VEC + e]);
        mask |= 1u << e;
      }
    }
    return mask;
  }
};

DEV_INLINE u64 wave_incl_scan(u64 v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u64 o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// Exact t-th largest by radix descent. COUNT: every column with key >=
// floor_key counts 1 and t = t0 (the k of top-k). Otherwise a column
// weighs weight_q and t = ceil(top_p * total), total being their sum: the
// result is the largest key whose columns at or above it weigh >= t.
// sel: three LDS words. Returns floor_key when the total is 0. Called by
// all ST threads; contains block barriers.
template <typename T, bool COUNT>
DEV_INLINE uint32_t radix_descend(const Row<T>& row, uint32_t floor_key,
                                  u64 t0, float top_p, float m, float c,
                                  u64* hist, u64* tot, u64* sel) {
  constexpr int VEC = Row<T>::VEC;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t prefix = 0;
  u64 t = t0;
  bool empty = false;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 256 * RC; i += ST) hist[i] = 0;
    if (tid == 0) {
      sel[0] = 0;
      sel[1] = t;
    }
    __syncthreads();
    for (int g = tid; g < row.ngroups; g += ST) {
      float z[VEC];
      const unsigned mask = row.load(g, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const uint32_t k = key_of(z[e]);
        const uint32_t hi =
            static_cast<uint32_t>(static_cast<u64>(k) >> (shift + 8));
        if (((mask >> e) & 1u) && k >= floor_key && hi == prefix) {
          const u64 v = COUNT ? 1ull : weight_q(z[e], m, c);
          if (v)
            atomicAdd(&hist[((k >> shift) & 255u) * RC + (lane & (RC - 1))],
                      v);
        }
      }
    }
    __syncthreads();
    if (tid < 256) {
      u64 s = 0;
#pragma unroll
      for (int r = 0; r < RC; ++r) s += hist[tid * RC + r];
      tot[tid] = s;
    }
    __syncthreads();
    if (wid == 0) {
      // lane l owns bins 255-4l .. 252-4l: highest values first
      u64 b[4], cum[5];
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = tot[255 - 4 * lane - e];
      const u64 s = b[0] + b[1] + b[2] + b[3];
      const u64 incl = wave_incl_scan(s, lane);
      const u64 total = __shfl(incl, 63, 64);
      if (pass == 0) {
        if (!COUNT) t = frac_target(top_p, total);
        if (lane == 0) sel[2] = total;
      }
      cum[0] = incl - s;
#pragma unroll
      for (int e = 0; e < 4; ++e) cum[e + 1] = cum[e] + b[e];
      if (t > cum[0] && t <= cum[4]) {
        int e = 0;
        u64 ce = cum[0];
#pragma unroll
        for (int j = 1; j < 4; ++j)
          if (t > cum[j]) {
            e = j;
            ce = cum[j];
          }
        sel[0] = static_cast<u64>(255 - 4 * lane - e);
        sel[1] = t - ce;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | static_cast<uint32_t>(sel[0]);
    t = sel[1];
    if (pass == 0) empty = sel[2] == 0;
    __syncthreads();
  }
  return empty ? floor_key : prefix;
}

template <typename T>
__global__ __launch_bounds__(ST) void sample_logits_kernel(
    const T* __restrict__ logits, int64_t row_stride, int vocab, float c,
    int top_k, float top_p, uint64_t seed, const int64_t* __restrict__ step,
    const float* __restrict__ u_in, int64_t* __restrict__ out,
    float* __restrict__ tau_out) {
  constexpr int VEC = Row<T>::VEC;
  __shared__ u64 hist[256 * RC];
  __shared__ u64 tot[256];
  __shared__ u64 wtot[SW];
  __shared__ u64 sel[3];
  __shared__ float red_m[SW];
  __shared__ uint32_t red_k[SW];
  __shared__ int pick[2];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const Row<T> row(logits + static_cast<int64_t>(b) * row_stride, vocab);

  // row maximum (NaN ignored) and smallest key
  float m = -INFINITY;
  uint32_t kmin = 0xffffffffu;
  for (int g = tid; g < row.ngroups; g += ST) {
    float z[VEC];
    const unsigned mask = row.load(g, z);
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if ((mask >> e) & 1u) {
        m = fmaxf(m, z[e]);
        const uint32_t k = key_of(z[e]);
        kmin = k < kmin ? k : kmin;
      }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    m = fmaxf(m, __shfl_xor(m, off, 64));
    const uint32_t o = __shfl_xor(kmin, off, 64);
    kmin = o < kmin ? o : kmin;
  }
  if (lane == 0) {
    red_m[wid] = m;
    red_k[wid] = kmin;
  }
  if (tid == 0) {
    pick[0] = INT_MAX;
    pick[1] = -1;
  }
  __syncthreads();
  for (int i = 0; i < SW; ++i) {
    m = fmaxf(m, red_m[i]);
    kmin = red_k[i] < kmin ? red_k[i] : kmin;
  }

  // thresholds (kernel arguments only: block-uniform branches)
  uint32_t ktau = 0;
  if (top_k > 0 && top_k < vocab)
    ktau = radix_descend<T, true>(row, 0u, static_cast<u64>(top_k), 0.0f, m,
                                  c, hist, tot, sel);
  if (top_p < 1.0f)
    ktau = radix_descend<T, false>(row, ktau, 0, top_p, m, c, hist, tot, sel);
  ktau = ktau > kmin ? ktau : kmin;

  // the uniform of this (seed, row, position)
  float u;
  if (u_in != nullptr) {
    u = u_in[b];
  } else {
    Philox4 rng(seed, static_cast<uint64_t>(b),
                static_cast<uint64_t>(step[0]));
    u = u32_to_uniform(rng().x);
  }
  u = fminf(fmaxf(u, 1.0f / 33554432.0f), 1.0f);

  // draw: each wave owns a contiguous run of groups. First the waves'
  // totals, then the one wave whose range holds the target walks it.
  const int gpw = (row.ngroups + SW - 1) / SW;
  const int g_lo = wid * gpw;
  const int g_hi = (g_lo + gpw < row.ngroups) ? g_lo + gpw : row.ngroups;
  u64 wsum = 0;
  for (int g0 = g_lo; g0 < g_hi; g0 += 64) {
    const int g = g0 + lane;
    if (g < g_hi) {
      float z[VEC];
      const unsigned mask = row.load(g, z);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (((mask >> e) & 1u) && key_of(z[e]) >= ktau)
          wsum += weight_q(z[e], m, c);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) wsum += __shfl_xor(wsum, off, 64);
  if (lane == 0) wtot[wid] = wsum;
  __syncthreads();
  u64 W = 0, base = 0;
  for (int i = 0; i < SW; ++i) {
    if (i == wid) base = W;
    W += wtot[i];
  }
  const u64 tq = frac_target(u, W);

  // W > 0: exactly one wave has base < tq <= base + wsum. W == 0 (only a
  // row of NaN): nothing is reached, every wave looks for the last kept
  // column.
  if (W == 0 || (base < tq && tq <= base + wsum)) {
    int found = INT_MAX, last = -1;
    for (int g0 = g_lo; g0 < g_hi; g0 += 64) {
      const int g = g0 + lane;
      u64 q[VEC];
      unsigned kept = 0;
      u64 s = 0;
#pragma unroll
      for (int e = 0; e < VEC; ++e) q[e] = 0;
      if (g < g_hi) {
        float z[VEC];
        const unsigned mask = row.load(g, z);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (((mask >> e) & 1u) && key_of(z[e]) >= ktau) {
            kept |= 1u << e;
            q[e] = weight_q(z[e], m, c);
            s += q[e];
          }
      }
      const u64 incl = wave_incl_scan(s, lane);
      u64 run = base + (incl - s);
      const int i0 = g * VEC - row.a;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        run += q[e];
        if (q[e] != 0 && run >= tq && found == INT_MAX) found = i0 + e;
        if ((kept >> e) & 1u) last = i0 + e;
      }
      base += __shfl(incl, 63, 64);
      if (base >= tq && W != 0) break;   // wave-uniform
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int f = __shfl_xor(found, off, 64);
      const int l = __shfl_xor(last, off, 64);
      found = f < found ? f : found;
      last = l > last ? l : last;
    }
    if (lane == 0) {
      atomicMin(&pick[0], found);
      atomicMax(&pick[1], last);
    }
  }
  __syncthreads();
  if (tid == 0) {
    int tok = pick[0] != INT_MAX ? pick[0] : pick[1];
    tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
    out[b] = tok;
    if (tau_out != nullptr) tau_out[b] = val_of(ktau);
  }
}

}  // namespace

void sample_logits(const void* logits, bool logits_bf16, int64_t row_stride,
                   int B, int vocab, float temperature, int top_k,
                   float top_p, uint64_t seed, const int64_t* step,
                   const float* u, int64_t* out, float* tau,
                   hipStream_t stream) {
  if (B < 1 || vocab < 1 || vocab > (1 << 22) || !(temperature > 0.0f) ||
      top_k < 0 || !(top_p > 0.0f))
    throw std::runtime_error(
        "sample_logits: need B >= 1, 1 <= vocab <= 2^22, temperature > 0, "
        "top_k >= 0, top_p > 0");
  if ((u == nullptr) == (step == nullptr))
    throw std::runtime_error("sample_logits: exactly one of u and step");
  if (out == nullptr || logits == nullptr)
    throw std::runtime_error("sample_logits: null logits or out");
  // (z - m) / T in exp2 units; formed in double, rounded once
  const float c = static_cast<float>(1.4426950408889634 /
                                     static_cast<double>(temperature));
  if (logits_bf16)
    hipLaunchKernelGGL(sample_logits_kernel<uint16_t>, dim3(B), dim3(ST), 0,
                       stream, static_cast<const uint16_t*>(logits),
                       row_stride, vocab, c, top_k, top_p, seed, step, u, out,
                       tau);
  else
    hipLaunchKernelGGL(sample_logits_kernel<float>, dim3(B), dim3(ST), 0,
                       stream, static_cast<const float*>(logits), row_stride,
                       vocab, c, top_k, top_p, seed, step, u, out, tau);
}

}  // namespace tepdist
