// Fused MoE routing, dispatch and combine for gfx950.
//
// Route (three plain launches in stream order, no workgroup waits on
// another, no atomics):
//   1. moe_topk_kernel     one thread per token, 256-token chunks. Picks
//      the k largest gates (ties to the lower expert), ranks every
//      selection among the chunk's earlier tokens of the same expert with
//      ballot + popcount of the lower lanes, and writes the per-chunk
//      per-expert counts to a workspace [chunks, E]. `slot` holds the
//      in-chunk rank for the moment.
//   2. moe_scan_kernel     one block: exclusive scan of the workspace over
//      the chunks (one wave per expert, shuffle scan with a carry), totals
//      to counts[E].
//   3. moe_slot_kernel     slot = e*C + chunk offset + in-chunk rank (or -1
//      past the capacity), src[slot] = t*k + j, and -1 into every slot of
//      src at or above min(counts[e], C). Filled and empty slots are
//      disjoint, so every element of src has exactly one writer.
//
// Rows: dispatch fwd / combine bwd (dy) gather ONE row per slot through
// src; dispatch bwd / combine fwd gather up to k rows per token through
// slot and sum them in fp32 in the order j = 0..k-1. All row traffic is
// 16-byte loads and stores (8 bf16), one per thread. Indices are range
// checked against the buffer they address, and an entry that fails the
// check counts as empty/dropped, so no map content can lead outside a
// buffer. Dropped and empty entries are switched off by selects, never by
// a multiplication with zero.

#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace tepdist {

namespace {

constexpr int NT = 256;
constexpr int NW = NT / WAVE;
constexpr int KMAX = 4;
constexpr int EMAX = 64;
constexpr int FILL_PER_BLOCK = NT * 8;  // src slots marked per block
constexpr int LPT = 16;                 // lanes per token in the dw kernel

DEV_INLINE float to_f(float v) { return v; }
DEV_INLINE float to_f(bf16_t v) { return bf2f(v); }

// One selection step: the largest gate among the experts not picked yet.
// `take` is false whenever the comparison involves a NaN, so a NaN gate is
// only ever chosen as "first free expert": the result is always a free
// index in [0, E), whatever the gates hold.
DEV_INLINE void consider(int e, float v, uint64_t picked, int& best,
                         float& bv) {
  const bool free_e = !((picked >> e) & 1ull);
  const bool take = free_e && (best < 0 || v > bv);
  best = take ? e : best;
  bv = take ? v : bv;
}

// EREG > 0: the token's gates live in EREG registers (E <= EREG);
// EREG == 0: they are re-read from memory (L1/L2 hits) for each of the k
// selection steps.
template <typename T, int EREG>
__launch_bounds__(NT) __global__
void moe_topk_kernel(const T* __restrict__ gates, int* __restrict__ topi,
                     int* __restrict__ rank_out, int* __restrict__ chunk_cnt,
                     int Tn, int E, int k, int vec8) {
  __shared__ int wcnt[NW][EMAX];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int t = blockIdx.x * NT + threadIdx.x;
  const bool live = t < Tn;

  uint64_t picked = 0;
  int sel[KMAX] = {-1, -1, -1, -1};
  if (live) {
    const T* g = gates + (int64_t)t * E;
    if constexpr (EREG > 0) {
      float gv[EREG];
      bool loaded = false;
      if constexpr (sizeof(T) == 2 && EREG == 8) {
        if (vec8) {  // E == 8 and a 16-byte aligned base: one load per token
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(g);
#pragma unroll
          for (int e = 0; e < 8; ++e) gv[e] = bf2f(v[e]);
          loaded = true;
        }
      }
      if (!loaded) {
#pragma unroll
        for (int e = 0; e < EREG; ++e) gv[e] = e < E ? to_f(g[e]) : 0.f;
      }
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        if (j < k) {
          int best = -1;
          float bv = 0.f;
#pragma unroll
          for (int e = 0; e < EREG; ++e)
            if (e < E) consider(e, gv[e], picked, best, bv);
          picked |= 1ull << best;
          sel[j] = best;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        if (j < k) {
          int best = -1;
          float bv = 0.f;
          for (int e = 0; e < E; ++e)
            consider(e, to_f(g[e]), picked, best, bv);
          picked |= 1ull << best;
          sel[j] = best;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j < k) topi[(int64_t)t * k + j] = sel[j];
  }

  // rank among the earlier tokens of the wave, per expert
  const uint64_t lower = (1ull << lane) - 1ull;
  int rank[KMAX] = {0, 0, 0, 0};
  for (int e = 0; e < E; ++e) {
    const bool c = (picked >> e) & 1ull;
    const uint64_t m = __ballot(c);
    if (lane == 0) wcnt[wid][e] = __popcll(m);
    if (c) {
      const int r = __popcll(m & lower);
#pragma unroll
      for (int j = 0; j < KMAX; ++j) rank[j] = sel[j] == e ? r : rank[j];
    }
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j < k) {
        int r = rank[j];
        for (int w = 0; w < wid; ++w) r += wcnt[w][sel[j]];
        rank_out[(int64_t)t * k + j] = r;
      }
    }
  }
  if ((int)threadIdx.x < E) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += wcnt[w][threadIdx.x];
    chunk_cnt[(int64_t)blockIdx.x * E + threadIdx.x] = s;
  }
}

// In place: chunk_cnt[c][e] := sum of chunk_cnt[c'][e] over c' < c;
// counts[e] := the total. Wave w owns experts w, w + NW, ...
__launch_bounds__(NT) __global__
void moe_scan_kernel(int* __restrict__ chunk_cnt, int* __restrict__ counts,
                     int nchunks, int E) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  for (int e = wid; e < E; e += NW) {
    int carry = 0;
    for (int base = 0; base < nchunks; base += WAVE) {
      const int c = base + lane;
      const bool in = c < nchunks;
      const int v = in ? chunk_cnt[(int64_t)c * E + e] : 0;
      int incl = v;
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        incl += lane >= off ? o : 0;
      }
      if (in) chunk_cnt[(int64_t)c * E + e] = carry + incl - v;
      carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) counts[e] = carry;
  }
}

__launch_bounds__(NT) __global__
void moe_slot_kernel(const int* __restrict__ topi, int* __restrict__ slot,
                     int* __restrict__ src, const int* __restrict__ chunk_off,
                     const int* __restrict__ counts, int Tn, int E, int k,
                     int C, int EC, int nchunks) {
  const int t = blockIdx.x * NT + threadIdx.x;
  if ((int)blockIdx.x < nchunks && t < Tn) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j < k) {
        const int64_t f = (int64_t)t * k + j;
        const int e = topi[f];
        // 64-bit: a rank can approach T while C is large
        const int64_t pos =
            (int64_t)slot[f] + chunk_off[(int64_t)blockIdx.x * E + e];
        const bool keep = pos < C;
        const int s = keep ? e * C + (int)pos : -1;
        slot[f] = s;
        if (keep) src[s] = (int)f;
      }
    }
  }
  // mark the slots nobody fills: positions at or above min(counts[e], C)
  const int64_t i0 = (int64_t)blockIdx.x * FILL_PER_BLOCK;
#pragma unroll
  for (int u = 0; u < FILL_PER_BLOCK / NT; ++u) {
    const int64_t i = i0 + u * NT + threadIdx.x;
    if (i < EC) {
      const unsigned e = (unsigned)i / (unsigned)C;  // EC < 2^31
      const int p = (int)((unsigned)i - e * (unsigned)C);
      if (p >= counts[e]) src[i] = -1;
    }
  }
}

// out[s, :] = (w[src[s]] *) in[src[s] / k, :] for a valid src[s], else 0.
// One 16-byte vector per thread; n_flat = rows of `in` times k.
template <bool WEIGHTED>
__launch_bounds__(NT) __global__
void moe_gather_rows_kernel(const bf16_t* __restrict__ in,
                            const int* __restrict__ src,
                            const float* __restrict__ w,
                            bf16_t* __restrict__ out, unsigned total,
                            unsigned dv, int k, int n_flat) {
  const unsigned idx = blockIdx.x * NT + threadIdx.x;  // total < 2^31
  if (idx >= total) return;
  const unsigned s = idx / dv;
  const unsigned c = idx - s * dv;
  const int f = src[s];
  const bool ok = (unsigned)f < (unsigned)n_flat;
  const int fc = ok ? f : 0;
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(
      in + ((int64_t)(fc / k) * dv + c) * 8);
  bf16x8 o;
  if constexpr (WEIGHTED) {
    const float wt = w[fc];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      o[i] = ok ? f2bf(wt * bf2f(v[i])) : f2bf(0.f);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = ok ? v[i] : f2bf(0.f);
  }
  *reinterpret_cast<bf16x8*>(out + (int64_t)idx * 8) = o;
}

// out[t, :] = sum over valid j of (w[t, j] *) in[slot[t, j], :], fp32
// accumulation in the order j = 0..k-1, rounded to bf16 once. The k row
// loads are issued before the first use; an invalid entry re-reads row 0
// and is dropped by a select.
template <bool WEIGHTED>
__launch_bounds__(NT) __global__
void moe_reduce_rows_kernel(const bf16_t* __restrict__ in,
                            const int* __restrict__ slot,
                            const float* __restrict__ w,
                            bf16_t* __restrict__ out, unsigned total,
                            unsigned dv, int k, int EC) {
  const unsigned idx = blockIdx.x * NT + threadIdx.x;  // total < 2^31
  if (idx >= total) return;
  const unsigned t = idx / dv;
  const unsigned c = idx - t * dv;
  bf16x8 v[KMAX];
  bool ok[KMAX];
  float wt[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    ok[j] = false;
    wt[j] = 1.f;
    if (j < k) {
      const int s = slot[(int64_t)t * k + j];
      ok[j] = (unsigned)s < (unsigned)EC;
      const int sc = ok[j] ? s : 0;
      v[j] = *reinterpret_cast<const bf16x8*>(in + ((int64_t)sc * dv + c) * 8);
      if constexpr (WEIGHTED) wt[j] = w[(int64_t)t * k + j];
    }
  }
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < k) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float a = WEIGHTED ? __builtin_fmaf(wt[j], bf2f(v[j][i]), acc[i])
                                 : acc[i] + bf2f(v[j][i]);
        acc[i] = ok[j] ? a : acc[i];
      }
    }
  }
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f2bf(acc[i]);
  *reinterpret_cast<bf16x8*>(out + (int64_t)idx * 8) = o;
}

// dw[t, j] = dot(y[slot[t, j], :], dout[t, :]) in fp32, 0 for an invalid
// slot. LPT lanes per token; lane i owns vectors i, i + LPT, ... of the row,
// partial sums meet through __shfl_xor within the lane group.
__launch_bounds__(NT) __global__
void moe_combine_dw_kernel(const bf16_t* __restrict__ y,
                           const bf16_t* __restrict__ dout,
                           const int* __restrict__ slot,
                           float* __restrict__ dw, int Tn, int dv, int k,
                           int EC) {
  const int sub = threadIdx.x % LPT;
  const int64_t t = (int64_t)blockIdx.x * (NT / LPT) + threadIdx.x / LPT;
  const bool live = t < Tn;
  int sc[KMAX];
  bool ok[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    const int s = (live && j < k) ? slot[t * k + j] : -1;
    ok[j] = (unsigned)s < (unsigned)EC;
    sc[j] = ok[j] ? s : 0;
  }
  float acc[KMAX] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    for (int c = sub; c < dv; c += LPT) {
      const bf16x8 g =
          *reinterpret_cast<const bf16x8*>(dout + (t * dv + c) * 8);
#pragma unroll
      for (int j = 0; j < KMAX; ++j) {
        if (ok[j]) {
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(
              y + ((int64_t)sc[j] * dv + c) * 8);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            acc[j] = __builtin_fmaf(bf2f(v[i]), bf2f(g[i]), acc[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
#pragma unroll
    for (int off = LPT / 2; off > 0; off >>= 1)
      acc[j] += __shfl_xor(acc[j], off, 64);
  }
  if (live && sub == 0) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j < k) dw[t * k + j] = ok[j] ? acc[j] : 0.f;
  }
}

bool aligned(const void* p, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

void check_common(const char* op, int T, int k, int64_t EC) {
  if (T < 1 || k < 1 || k > KMAX || (int64_t)T * k >= (1ll << 31))
    throw std::runtime_error(std::string(op) +
                             ": need T >= 1, 1 <= k <= 4, T*k < 2^31");
  if (EC < 1 || EC >= (1ll << 31))
    throw std::runtime_error(std::string(op) + ": need 1 <= E*C < 2^31");
}

// rows * (d / 8) vectors, one per thread
unsigned row_grid(const char* op, int64_t rows, int d) {
  if (d < 8 || d % 8)
    throw std::runtime_error(std::string(op) +
                             ": row width must be a positive multiple of 8");
  const int64_t total = rows * (d / 8);  // 32-bit index math in the kernels
  if (total >= (1ll << 31))
    throw std::runtime_error(std::string(op) +
                             ": rows * d / 8 must stay below 2^31");
  return (unsigned)((total + NT - 1) / NT);
}

}  // namespace

int64_t moe_route_ws_ints(int T, int E) {
  return ((int64_t)T + NT - 1) / NT * E;
}

void moe_route(const void* gates, bool gates_fp32, int* topi, int* slot,
               int* src, int* counts, int* ws, int T, int E, int k, int C,
               hipStream_t stream) {
  if (E < 2 || E > EMAX)
    throw std::runtime_error("moe_route: need 2 <= E <= 64");
  if (k < 1 || k > KMAX || k > E)
    throw std::runtime_error("moe_route: need 1 <= k <= min(4, E)");
  if (C < 1) throw std::runtime_error("moe_route: need C >= 1");
  const int64_t EC = (int64_t)E * C;
  check_common("moe_route", T, k, EC);
  if (!gates || !topi || !slot || !src || !counts || !ws)
    throw std::runtime_error("moe_route: null operand");
  if (!aligned(gates, gates_fp32 ? 4 : 2) || !aligned(topi, 4) ||
      !aligned(slot, 4) || !aligned(src, 4) || !aligned(counts, 4) ||
      !aligned(ws, 4))
    throw std::runtime_error("moe_route: misaligned operand");

  const int nchunks = (T + NT - 1) / NT;
  const int vec8 = (!gates_fp32 && E == 8 && aligned(gates, 16)) ? 1 : 0;
#define MR_TOPK(TT, ER)                                                      \
  hipLaunchKernelGGL((moe_topk_kernel<TT, ER>), dim3(nchunks), dim3(NT), 0,  \
                     stream, static_cast<const TT*>(gates), topi, slot, ws,  \
                     T, E, k, vec8)
  if (gates_fp32) {
    if (E <= 8) MR_TOPK(float, 8); else MR_TOPK(float, 0);
  } else {
    if (E <= 8) MR_TOPK(bf16_t, 8); else MR_TOPK(bf16_t, 0);
  }
#undef MR_TOPK
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(NT), 0, stream, ws,
                     counts, nchunks, E);
  const int64_t fill_blocks = (EC + FILL_PER_BLOCK - 1) / FILL_PER_BLOCK;
  const unsigned grid3 =
      (unsigned)(fill_blocks > nchunks ? fill_blocks : nchunks);
  hipLaunchKernelGGL(moe_slot_kernel, dim3(grid3), dim3(NT), 0, stream, topi,
                     slot, src, ws, counts, T, E, k, C, (int)EC, nchunks);
}

void moe_gather_rows_bf16(const void* in, const int* src, const float* w,
                          void* out, int T, int k, int64_t EC, int d,
                          hipStream_t stream) {
  check_common("moe_gather_rows", T, k, EC);
  const unsigned grid = row_grid("moe_gather_rows", EC, d);
  if (!in || !src || !out)
    throw std::runtime_error("moe_gather_rows: null operand");
  if (!aligned(in, 16) || !aligned(out, 16) || !aligned(src, 4) ||
      !aligned(w, 4))
    throw std::runtime_error("moe_gather_rows: rows must be 16-byte aligned");
  const unsigned dv = d / 8;
  const unsigned total = (unsigned)(EC * dv);
  const bf16_t* ip = static_cast<const bf16_t*>(in);
  bf16_t* op = static_cast<bf16_t*>(out);
  if (w)
    hipLaunchKernelGGL(moe_gather_rows_kernel<true>, dim3(grid), dim3(NT), 0,
                       stream, ip, src, w, op, total, dv, k, T * k);
  else
    hipLaunchKernelGGL(moe_gather_rows_kernel<false>, dim3(grid), dim3(NT), 0,
                       stream, ip, src, w, op, total, dv, k, T * k);
}

void moe_reduce_rows_bf16(const void* in, const int* slot, const float* w,
                          void* out, int T, int k, int64_t EC, int d,
                          hipStream_t stream) {
  check_common("moe_reduce_rows", T, k, EC);
  const unsigned grid = row_grid("moe_reduce_rows", T, d);
  if (!in || !slot || !out)
    throw std::runtime_error("moe_reduce_rows: null operand");
  if (!aligned(in, 16) || !aligned(out, 16) || !aligned(slot, 4) ||
      !aligned(w, 4))
    throw std::runtime_error("moe_reduce_rows: rows must be 16-byte aligned");
  const unsigned dv = d / 8;
  const unsigned total = (unsigned)((int64_t)T * dv);
  const bf16_t* ip = static_cast<const bf16_t*>(in);
  bf16_t* op = static_cast<bf16_t*>(out);
  if (w)
    hipLaunchKernelGGL(moe_reduce_rows_kernel<true>, dim3(grid), dim3(NT), 0,
                       stream, ip, slot, w, op, total, dv, k, (int)EC);
  else
    hipLaunchKernelGGL(moe_reduce_rows_kernel<false>, dim3(grid), dim3(NT), 0,
                       stream, ip, slot, w, op, total, dv, k, (int)EC);
}

void moe_combine_dw_bf16(const void* y, const void* dout, const int* slot,
                         float* dw, int T, int k, int64_t EC, int d,
                         hipStream_t stream) {
  check_common("moe_combine_dw", T, k, EC);
  row_grid("moe_combine_dw", T, d);
  if (!y || !dout || !slot || !dw)
    throw std::runtime_error("moe_combine_dw: null operand");
  if (!aligned(y, 16) || !aligned(dout, 16) || !aligned(slot, 4) ||
      !aligned(dw, 4))
    throw std::runtime_error("moe_combine_dw: rows must be 16-byte aligned");
  const unsigned grid = (unsigned)(((int64_t)T + NT / LPT - 1) / (NT / LPT));
  hipLaunchKernelGGL(moe_combine_dw_kernel, dim3(grid), dim3(NT), 0, stream,
                     static_cast<const bf16_t*>(y),
                     static_cast<const bf16_t*>(dout), slot, dw, T, d / 8, k,
                     (int)EC);
}

}  // namespace tepdist
