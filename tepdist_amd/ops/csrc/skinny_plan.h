// Host-side plan of one skinny-M (decode-step) linear: y[M, N] = x[M, K] .
// W[N, K]^T with 1 <= M <= 64. Plain C++17, no HIP include, like
// gemm_plan.h: skinny_gemm.hip launches what this returns, the extension
// binds it as `skinny_plan`, and a stand-alone host program can compile it
// alone. Coverage and launch shape of the skinny path are decided here and
// nowhere else.
#pragma once

#include <algorithm>
#include <cstdint>

namespace tepdist {

// Epilogues of the skinny kernels, on the fp32 sum, one rounding to bf16.
enum {
  SK_NONE = 0,
  SK_BIAS = 1,      // + bias[n]
  SK_BIAS_GELU = 2, // gelu(. + bias[n]), tanh form; no pre-activation output
  SK_RES = 3,       // + r[m, n]
  SK_BIAS_RES = 4   // + bias[n] + r[m, n]
};

struct SkinnyPlan {
  int mt;               // 16-token fragments per weight fragment: 1, 2, 4
  int rows;             // weight rows a block owns (per matrix when dual)
  int waves;            // waves per block; wave w owns K-steps w, w + waves...
  int k_per_wave;       // K elements of the largest share (wave 0's)
  int split_k;          // grid-level split: always 1 (not built)
  const char* why_not;  // set when the call is not covered, else nullptr
};

namespace skinny {
constexpr int KSTEP = 64;       // K elements of one step (two MFMAs)
constexpr int MAX_M = 64;
constexpr int MAX_WAVES = 8;
constexpr int WANT_WAVES = 1024;  // 4 per CU: enough 16-byte loads in flight
constexpr int WIDE_TILES = 1024;  // from here on a block takes 32 rows
}  // namespace skinny

// ldx / ldw: row strides of x and W in elements (ldw also W_up's when dual).
// The bases of x and W must be 16-byte aligned too; the launcher checks
// that, since only it sees them. The residual may have any row stride.
inline SkinnyPlan skinny_plan(int M, int N, int K, int64_t ldx, int64_t ldw,
                              int epi, bool dual) {
  using namespace skinny;
  const SkinnyPlan no = {0, 0, 0, 0, 1, nullptr};
  auto refuse = [&](const char* why) {
    SkinnyPlan p = no;
    p.why_not = why;
    return p;
  };
  if (epi < SK_NONE || epi > SK_BIAS_RES) return refuse("epi must be 0..4");
  if (dual && epi != SK_NONE)
    return refuse("the dual SwiGLU kernel has no bias or residual epilogue");
  if (M < 1 || M > MAX_M) return refuse("M must be in 1..64");
  if (N < 1) return refuse("N must be positive");
  if (K < KSTEP || K % KSTEP != 0)
    return refuse("K must be a positive multiple of 64");
  if (ldx < K || ldw < K || (ldx & 7) || (ldw & 7))
    return refuse("rows of x and W must be 16-byte aligned (strides that are "
                  "multiples of 8 elements, at least K)");

  SkinnyPlan p = no;
  p.mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
  // A block re-reads all of x from L2, so fewer, taller blocks cut that
  // traffic; but a small N needs every block it can get. 32 rows only where
  // 16-row tiles alone already give WANT_WAVES blocks. The dual kernel
  // streams two matrices per block and stays at 16 rows of each.
  const int tiles = (N + 15) / 16;
  p.rows = (!dual && tiles >= WIDE_TILES) ? 32 : 16;
  const int blocks = (N + p.rows - 1) / p.rows;
  // waves split K inside the block: as many as fill the chip, each with at
  // least one K-step
  int w = 1;
  while (w < MAX_WAVES && blocks * w < WANT_WAVES) w *= 2;
  const int ksteps = K / KSTEP;
  p.waves = std::min(w, ksteps);
  p.k_per_wave = (ksteps + p.waves - 1) / p.waves * KSTEP;
  return p;
}

}  // namespace tepdist
