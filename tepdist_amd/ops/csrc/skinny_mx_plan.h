// Host-side plan of one skinny-M (decode-step) linear on MX weights:
// y[M, N] = x[M, K] . dq(W)[N, K]^T with 1 <= M <= 64, W stored as OCP MX
// codes (e2m1 or e4m3) and one e8m0 scale byte per 32 k (ops/mx.py). Plain
// C++17, no HIP include, like skinny_plan.h, whose epilogue enum and
// constants it shares: skinny_mx_gemm.hip launches what this returns and the
// extension binds it as `skinny_mx_plan`. Coverage and launch shape of the
// MX path are decided here and nowhere else.
#pragma once

#include <algorithm>
#include <cstdint>

#include "skinny_plan.h"

namespace tepdist {

struct SkinnyMxPlan {
  int mt;               // 16-token fragments per weight fragment: 1, 2, 4
  int rows;             // weight rows a block owns (per matrix when dual)
  int waves;            // waves per block; wave w owns K-steps w, w + waves...
  int k_per_wave;       // K elements of the largest share (wave 0's)
  int unroll;           // K-steps in flight per register set
  const char* why_not;  // set when the call is not covered, else nullptr
};

namespace skinny_mx {
constexpr int KSTEP = 128;  // K elements of one step: four MFMAs, and per
                            // lane exactly one MX block of 32

// K-steps in flight per register set. A step holds, per lane, 16 MT VGPRs
// of x (four 16-byte loads per token fragment) and per weight tile bits
// VGPRs of codes (one 16-byte load for e2m1, two for e4m3) plus the scale
// byte. A step is two of the bf16 kernel's, so its 2-step threshold of 40
// VGPRs becomes 48 for two steps of 128: at most 96 VGPRs per set, 192 for
// the ping-pong pair, which leaves room for the accumulators and the
// dequantized fragments below 256. Four steps (what the rule would give
// e2m1 at MT = 1, one tile: 21 VGPRs) are not used: at the flagship K of
// 1024..2048 a wave of eight owns one or two steps, so the look-ahead only
// re-read x, and measured 7.5 us against e4m3's 5.8 us at N 3072, K 2048,
// M 1.
constexpr int unroll(int T, int MT, int bits) {
  const int s = 16 * MT + T * (bits + 1);
  return s <= 48 ? 2 : 1;
}
}  // namespace skinny_mx

// bits: 4 (e2m1) or 8 (e4m3). ld_codes / ld_scales: row strides of the code
// and scale arrays in bytes (also W_up's when dual). Bases of x, codes and
// scales and the rows of x are checked by the launcher, which alone sees
// them.
inline SkinnyMxPlan skinny_mx_plan(int M, int N, int K, int bits,
                                   int64_t ld_codes, int64_t ld_scales,
                                   int epi, bool dual) {
  using namespace skinny;
  const SkinnyMxPlan no = {0, 0, 0, 0, 0, nullptr};
  auto refuse = [&](const char* why) {
    SkinnyMxPlan p = no;
    p.why_not = why;
    return p;
  };
  if (bits != 4 && bits != 8)
    return refuse("bits must be 4 (mxfp4) or 8 (mxfp8)");
  if (epi < SK_NONE || epi > SK_BIAS_RES) return refuse("epi must be 0..4");
  if (dual && epi != SK_NONE)
    return refuse("the dual SwiGLU kernel has no bias or residual epilogue");
  if (M < 1 || M > MAX_M) return refuse("M must be in 1..64");
  if (N < 1) return refuse("N must be positive");
  if (K < skinny_mx::KSTEP || K % skinny_mx::KSTEP != 0)
    return refuse("K must be a positive multiple of 128");
  if (ld_codes < (int64_t)K * bits / 8 || (ld_codes & 15))
    return refuse("code rows must be 16-byte aligned (a byte stride that is "
                  "a multiple of 16, at least K * bits / 8)");
  if (ld_scales < K / 32 || (ld_scales & 3))
    return refuse("scale rows must be 4-byte aligned (a byte stride that is "
                  "a multiple of 4, at least K / 32)");

  SkinnyMxPlan p = no;
  p.mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
  // rows and waves by the bf16 kernel's rules (skinny_plan.h): x traffic
  // per block is what it was, only the weight bytes shrank
  const int tiles = (N + 15) / 16;
  p.rows = (!dual && tiles >= WIDE_TILES) ? 32 : 16;
  const int blocks = (N + p.rows - 1) / p.rows;
  int w = 1;
  while (w < MAX_WAVES && blocks * w < WANT_WAVES) w *= 2;
  const int ksteps = K / skinny_mx::KSTEP;
  p.waves = std::min(w, ksteps);
  p.k_per_wave = (ksteps + p.waves - 1) / p.waves * skinny_mx::KSTEP;
  p.unroll = skinny_mx::unroll(dual ? 2 : p.rows / 16, p.mt, bits);
  return p;
}

}  // namespace tepdist
