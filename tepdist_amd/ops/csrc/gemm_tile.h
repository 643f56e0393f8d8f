// Device-side pieces shared by the two hand GEMM kernels (gemm.hip,
// gemm256.hip): the epilogue codes and tile sizes (from gemm_plan.h), the
// swizzled [rows][64] LDS image (lds_frag.h), the global_load_lds pointer
// types and the XCD block remap.
#pragma once

#include "common.h"
#include "gemm_plan.h"
#include "lds_frag.h"

namespace tepdist {

// __builtin_amdgcn_global_load_lds operands (direct HBM->LDS DMA). The
// destination is wave-uniform base + lane*16B (lane-linear), so a swizzled
// image is staged by applying the XOR to the per-lane SOURCE address: LDS
// element (row, c) receives global k = c ^ (SWZ8(row) << 3).
typedef __attribute__((address_space(1))) const void* glds_src_t;
typedef __attribute__((address_space(3))) void* glds_dst_t;

// XCD-aware bijective block swizzle (guide T1): the dispatcher places block
// b on XCD b%8; remap so each XCD gets a CONTIGUOUS run of tiles
// (consecutive n-tiles share the A panel -> L2 hits stay on one XCD).
// Returns the tile index for block `bid` of an `nwg`-block grid.
DEV_INLINE int xcd_remap(unsigned bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

}  // namespace tepdist
