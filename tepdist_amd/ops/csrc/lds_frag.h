// Swizzled LDS tile images shared by the GEMM, transpose and flash-attention
// kernels and the fragment probe in debug.hip.
#pragma once

#include "common.h"

namespace tepdist {

// The swizzle: a row's 16B column slots are XORed with x(row) = the
// bit-reversed (row>>1)&7. The bit reversal puts the fragment-read service
// groups' row bit (row bit 1 under quad-strided 16-lane grouping, row bits
// 1..3 under contiguous grouping) into slot bits that the reads' own column
// spread does not already cover, making ds_read_b128 column reads
// conflict-free; writes stay <=2-way.
// A macro on purpose: as a function LLVM simplifies it on its own before
// inlining (it recognises the bit reversal), and the global_load_lds
// staging sites, which fold it into the thread-index shifts instead, come
// out with different address code and register counts.
#define SWZ8(row)                                     \
  ({                                                  \
    const int r1_ = (row) >> 1;                       \
    ((r1_ & 1) << 2) | (r1_ & 2) | ((r1_ >> 2) & 1);  \
  })

// LDS addressing for a [rows][C] bf16 image of unpadded rows, C in {64,128}.
template <int C>
DEV_INLINE int loff(int row, int col_e) {
  const int x = SWZ8(row);
  return row * C + (col_e ^ ((x << 3) & (C - 1)));
}

typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;

// A-fragment of the TRANSPOSE of a natural [rows][C] image (written through
// loff<C>), for mfma_f32_16x16x32_bf16 under the kernels' k-permuted order:
//   lane = 16g + i supplies MFMA row  m = image column 16*df + i
//   element e < 4  is k slot          image row 32*c + 4g + e
//   element e >= 4 is k slot          image row 32*c + 16 + 4g + (e - 4)
// i.e. frag[e] = image[32c + 16*(e>>2) + 4g + (e&3)][16df + i] — the same k
// order in which a 16x16 C-fragment pair (2c, 2c+1) packs into a B operand.
// Two ds_read_b64_tr_b16: within a 16-lane group, lane 4q+p supplies the
// address of row q, columns 4p..4p+3 of a 4-row x 16-column block, and lane
// i receives column i of the four rows. The swizzle moves whole 16B slots,
// so each lane's 4 elements stay contiguous and 8B-aligned. The gather
// crosses lanes: call only with all 64 lanes active (wave-uniform control
// flow), on an image whose rows are all written (zero-padded, never masked).
// Banks at C=64: a 32-lane half reads 8 consecutive rows x 32B; rows of
// equal parity differ in the XORed slot, odd/even rows sit 32 banks apart —
// conflict-free. At C=128 the odd/even rows share banks (2-way).
template <int C>
DEV_INLINE bf16x8 tr_frag(const bf16_t* img, int c, int df, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int row = 32 * c + 4 * g + (i >> 2);
  const int col = 16 * df + 4 * (i & 3);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4_ptr)(img + loff<C>(row, col)));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (lds_bf16x4_ptr)(img + loff<C>(row + 16, col)));
  bf16x8 f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = lo[e];
    f[e + 4] = hi[e];
  }
  return f;
}

}  // namespace tepdist
