// Diagnostic probes (not part of the training path).
// tr16_probe: determines the exact lane->element mapping of
// ds_read_b64_tr_b16 on this chip. LDS is filled with bf16(element_index);
// each lane reads at addr = base + (lane&15)*2B + (lane>>4)*128B and we dump
// the 4 returned values per lane, plus a uniform-address variant. (Those
// addresses are NOT the instruction's natural ones — lane 4q+p of a 16-lane
// group is meant to point at row q, columns 4p..4p+3 — so the pattern shows
// what unaligned addresses collapse to, not a usable fragment.)
// tr16_frag_probe: exercises tr_frag<C> (lds_frag.h), the transposed
// A-fragment read the flash kernels use, over a swizzled [64][C] image whose
// elements carry the bit pattern row*128 + col, and dumps every (c, df)
// fragment so a test can check each lane and element.

#include "common.h"
#include "kernels.h"
#include "lds_frag.h"

namespace tepdist {

namespace {

typedef __attribute__((address_space(3))) bf16x4* lds_tr_ptr;

__global__ void tr16_probe_kernel(float* out_pattern, float* out_uniform) {
  __shared__ bf16_t lds[512];
  for (int i = threadIdx.x; i < 512; i += blockDim.x)
    lds[i] = f2bf((float)i);
  __syncthreads();
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const bf16_t* p =
        &lds[0] + (lane & 15) + (lane >> 4) * 64;  // elements (2B each)
    bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr_ptr)p);
#pragma unroll
    for (int j = 0; j < 4; ++j) out_pattern[lane * 4 + j] = bf2f(v[j]);
    bf16x4 u = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr_ptr)&lds[0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) out_uniform[lane * 4 + j] = bf2f(u[j]);
  }
}

// out[c][df][lane][e] (int32) = bit pattern of element e of lane's
// tr_frag<C>(image, c, df); one wave, all lanes active at every read.
template <int C>
__global__ void tr16_frag_probe_kernel(int* out) {
  __shared__ __attribute__((aligned(16))) bf16_t img[64 * C];
  for (int i = threadIdx.x; i < 64 * C; i += 64) {
    const int row = i / C, col = i % C;
    reinterpret_cast<unsigned short*>(img)[loff<C>(row, col)] =
        (unsigned short)(row * 128 + col);
  }
  __syncthreads();
  const int lane = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int df = 0; df < C / 16; ++df) {
      const s16x8 bits =
          __builtin_bit_cast(s16x8, tr_frag<C>(img, c, df, lane));
#pragma unroll
      for (int e = 0; e < 8; ++e)
        out[((c * (C / 16) + df) * 64 + lane) * 8 + e] =
            (unsigned short)bits[e];
    }
}

}  // namespace

void tr16_frag_probe(int* out, int C, hipStream_t stream) {
  if (C == 64)
    hipLaunchKernelGGL(tr16_frag_probe_kernel<64>, dim3(1), dim3(64), 0,
                       stream, out);
  else if (C == 128)
    hipLaunchKernelGGL(tr16_frag_probe_kernel<128>, dim3(1), dim3(64), 0,
                       stream, out);
  else
    throw std::runtime_error("tr16_frag_probe: C must be 64 or 128");
  HIP_CHECK(hipGetLastError());
}

void tr16_probe(float* out_pattern, float* out_uniform, hipStream_t stream) {
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0, stream,
                     out_pattern, out_uniform);
  HIP_CHECK(hipGetLastError());
}

}  // namespace tepdist
