// Host-side plan of one tiled linear on MX weights: y[M, N] = x[M, K] .
// dq(W)[N, K]^T for any M >= 1, W stored as OCP MX codes (e2m1 or e4m3) and
// one e8m0 scale byte per 32 k (ops/mx.py). Plain C++17, no HIP include,
// like the other plans, whose epilogue enum it shares: mx_gemm.hip launches
// what this returns and the extension binds it as `mx_gemm_plan`. Coverage
// and tile choice of the tiled MX path are decided here and nowhere else.
#pragma once

#include <cstdint>

#include "skinny_plan.h"

namespace tepdist {

struct MxGemmPlan {
  int tile;             // block tile, square: 64 or 128
  int stages;           // LDS stages of the K pipeline
  int blocks;           // grid size
  const char* why_not;  // set when the call is not covered, else nullptr
};

namespace mx_tiled {
constexpr int KTILE = 128;  // K elements of one tile: four MFMAs, and per
                            // lane exactly one MX block of 32
constexpr int STAGES = 3;   // 145.5 KiB of the 160 at the 128-tile on e4m3;
                            // two blocks per CU at the 64-tile
constexpr int FILL = 256;   // the 128-tile wants one block per CU
}  // namespace mx_tiled

// bits: 4 (e2m1) or 8 (e4m3). ld_codes / ld_scales: row strides of the code
// and scale arrays in bytes. tile_override: 0 = the rule below, else 64 or
// 128. Bases and the rows of x, the residual and y are checked by the
// launcher, which alone sees them.
inline MxGemmPlan mx_gemm_plan(int M, int N, int K, int bits,
                               int64_t ld_codes, int64_t ld_scales, int epi,
                               int tile_override) {
  auto refuse = [](const char* why) { return MxGemmPlan{0, 0, 0, why}; };
  if (bits != 4 && bits != 8)
    return refuse("bits must be 4 (mxfp4) or 8 (mxfp8)");
  if (epi < SK_NONE || epi > SK_BIAS_RES) return refuse("epi must be 0..4");
  if (tile_override != 0 && tile_override != 64 && tile_override != 128)
    return refuse("tile must be 0 (the plan's choice), 64 or 128");
  if (M < 1 || N < 1) return refuse("M and N must be positive");
  if (K < mx_tiled::KTILE || K % mx_tiled::KTILE != 0)
    return refuse("K must be a positive multiple of 128");
  if (ld_codes < (int64_t)K * bits / 8 || (ld_codes & 15))
    return refuse("code rows must be 16-byte aligned (a byte stride that is "
                  "a multiple of 16, at least K * bits / 8)");
  if (ld_scales < K / 32 || (ld_scales & 3))
    return refuse("scale rows must be 4-byte aligned (a byte stride that is "
                  "a multiple of 4, at least K / 32)");

  auto grid = [&](int t) {
    return ((int64_t)M + t - 1) / t * (((int64_t)N + t - 1) / t);
  };
  // the 128-tile halves the LDS traffic per MFMA but runs one block per CU:
  // only where its grid covers the chip, else four times the blocks at 64
  const int tile = tile_override ? tile_override
                   : grid(128) >= mx_tiled::FILL ? 128 : 64;
  if (grid(tile) > INT32_MAX) return refuse("M * N is too large for one grid");
  return MxGemmPlan{tile, mx_tiled::STAGES, (int)grid(tile), nullptr};
}

}  // namespace tepdist
