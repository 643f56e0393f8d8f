// Host-side plan of one hand GEMM call: which kernel runs it, into how many
// K-chunks it splits and how long a chunk is. Plain C++17, no HIP include:
// gemm_bf16 (gemm.hip) launches what this returns, the extension binds it
// as `gemm_plan` for ops/hip.py, and a stand-alone host program can compile
// it alone. Every dispatch and split-K decision of the hand path is here
// and nowhere else.
#pragma once

#include <algorithm>
#include <cstdint>

namespace tepdist {

struct GemmPlan {
  int kernel;           // 256, 128, or 0 = no kernel accepts this call
  int split_k;          // 1 = no split
  int k_chunk;          // K elements per chunk; 0 when split_k == 1
  const char* why_not;  // set when kernel == 0, else nullptr
};

// Epilogues of the hand GEMM (the `epi` argument). The only definition:
// the kernels see it through gemm_tile.h.
enum {
  EPI_NONE = 0,
  EPI_BIAS = 1,       // + bias
  EPI_BIAS_GELU = 2,  // + bias, gelu; pre-activation written to c_pre
  EPI_GELU = 3,       // gelu; pre-activation written to c_pre
  // dgelu: C = (A@B) * gelu'(c_pre) — c_pre is the INPUT pre-activation
  // saved by the forward (the fusion hipBLASLt has no algorithms for on
  // gfx950, profiles/blaslt_epilogue_probe.md). 256 kernel only.
  EPI_DGELU = 4
};

namespace plan {
constexpr int T256 = 256;  // gemm256.hip tile (BM = BN)
constexpr int T128 = 128;  // gemm.hip tile (BM = BN)
constexpr int BK = 64;     // K-tile of both kernels
constexpr int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
}  // namespace plan

namespace plan {
// Split K when the (M, N) tile grid underfills the 256-CU chip and K is
// deep: aim at >= 512 blocks, prefer a whole number of 256-block
// generations so every CU stays busy to the end (48 blocks: x8 = 1.5
// generations -> x16 = 3 full), keep every chunk >= 2 K-tiles.
inline void split_for(int64_t blocks, int K, int epi, int batch,
                      int* split_k, int* k_chunk) {
  *split_k = 1;
  *k_chunk = 0;
  if (batch == 1 && epi == 0 && K >= 2048 && blocks < 384) {
    const int b = static_cast<int>(blocks), max_by_k = K / (2 * BK);
    int s = std::max(2, (512 + b - 1) / b);
    for (int cand = s; cand < std::min(17, max_by_k + 1); ++cand)
      if ((b * cand) % 256 == 0) {
        s = cand;
        break;
      }
    s = std::max(2, std::min({s, 16, max_by_k}));
    // Normalize to the number of chunks that are not empty once the chunk
    // is rounded up to whole K-tiles. This step rounds floor(K / s); when
    // K is not a multiple of 64 that can be one tile shorter than the
    // k_chunk below, and s = 16 then comes out as 17 (K = 2056: floor
    // gives 128, ceil(2056 / 128) = 17). Harmless, since k_chunk is
    // derived from the final count, and kept because changing it would
    // change results; it never happens when K % 64 == 0.
    const int64_t floor_chunk = cdiv(K / s, BK) * BK;
    *split_k = static_cast<int>(std::max<int64_t>(2, cdiv(K, floor_chunk)));
    *k_chunk = static_cast<int>(cdiv(cdiv(K, *split_k), BK) * BK);
  }
}

// The 256 kernel's pipeline needs >= 2 K-tiles in every chunk it runs, the
// last one included, and no empty chunk.
inline bool chunks_fit_256(int K, int split_k, int k_chunk) {
  if (K < 2 * BK) return false;
  if (split_k == 1) return true;
  return k_chunk >= 2 * BK && K % k_chunk != BK &&
         cdiv(K, k_chunk) == split_k;
}
}  // namespace plan

inline GemmPlan gemm_plan(int M, int N, int K, int lda, int ldb, bool a_kc,
                          bool b_kc, int epi, int batch) {
  using namespace plan;
  if (epi < EPI_NONE || epi > EPI_DGELU)
    return {0, 1, 0, "epi must be 0..4"};

  // The 256 kernel's tiling applies to whole tiles of two k-contiguous
  // operands. Row alignment is NOT part of this test: it only decides below
  // whether the 256 kernel accepts the call, so an unaligned canonical
  // shape keeps the 256-tiling block count and runs on the 128 kernel.
  const bool tiled = M % T256 == 0 && N % T256 == 0 && K % BK == 0;
  const bool canon = a_kc && b_kc && tiled;
  const bool aligned = (lda & 7) == 0 && (ldb & 7) == 0;  // 16-byte rows
  int split_k, k_chunk;

  // Two k-outer operands (wgrad: A stored [K][M], B stored [K][N]) run on
  // the 256 kernel in place, plain epilogue only, under the canonical
  // case's conditions and with its block count and split. A k-outer call
  // that misses any of them is planned below exactly as it always was.
  if (!a_kc && !b_kc && tiled && aligned && epi == EPI_NONE) {
    split_for(int64_t(M / T256) * (N / T256), K, epi, batch, &split_k,
              &k_chunk);
    if (chunks_fit_256(K, split_k, k_chunk))
      return {T256, split_k, k_chunk, nullptr};
  }

  const int64_t blocks = canon ? int64_t(M / T256) * (N / T256)
                               : cdiv(M, T128) * cdiv(N, T128);
  split_for(blocks, K, epi, batch, &split_k, &k_chunk);

  // Under split the 256 kernel has only the plain epilogue (split_for
  // never splits another).
  if (canon && aligned && chunks_fit_256(K, split_k, k_chunk))
    return {T256, split_k, k_chunk, nullptr};
  if (epi == EPI_DGELU)
    return {0, 1, 0,
            "epi 4 (dgelu) runs only on the 256 kernel: k-contiguous "
            "operands, M and N multiples of 256, K a multiple of 64 and "
            ">= 128, 16-byte-aligned rows"};
  return {T128, split_k, k_chunk, nullptr};
}

// Column sums of A (colsum[m] = sum over k of A[k][m], wgrad's bias
// gradient) come only from the 256 kernel on two k-outer operands: nullptr
// when plan `p` of a call with these layouts can produce them, else why not.
inline const char* colsum_why_not(const GemmPlan& p, bool a_kc, bool b_kc,
                                  int batch) {
  if (p.kernel != plan::T256 || a_kc || b_kc || batch != 1)
    return "colsum_out needs the 256 kernel on two k-outer operands (A "
           "stored [K][M], B stored [K][N], M and N multiples of 256, K a "
           "multiple of 64 and >= 128, 16-byte-aligned rows, epi 0, batch 1)";
  return nullptr;
}

// Floats of fp32 workspace that plan `p` of an [M, N] call needs, the only
// place that knows: split_k * M * N product partials when K is split, then,
// with column sums, one vector of M floats per part (split chunk, n-tile).
inline int64_t gemm_ws_floats(const GemmPlan& p, int M, int N, bool colsum) {
  int64_t n = p.split_k > 1 ? int64_t(p.split_k) * M * N : 0;
  if (colsum) n += int64_t(p.split_k) * (N / plan::T256) * M;
  return n;
}

}  // namespace tepdist
