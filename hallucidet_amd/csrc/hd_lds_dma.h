// LDS-DMA and XCD primitives shared by the convolution, GEMM and weight-gradient kernels.
#pragma once
#include "hd_common.h"

// Offsets that a raw BUFFER access finds out of range: the hardware returns zeros (LDS-DMA: writes zeros to LDS), so padding and
// ragged tails need no branch on the load path.
// OOB: beyond any tensor (all are < 4 GiB - 16), for an offset that is used as it stands.
// OOBB: an out-of-range lane keeps its offset at >= 2^31 whatever uniform offset is added later, for kernels whose tensors are
// < 2 GiB (their eligibility rules check it): the per-step address is then one add.
constexpr unsigned OOB = 0xFFFFFFF0u;
constexpr unsigned OOBB = 0x80000000u;

typedef __attribute__((address_space(3))) void lds_void;

// 16 bytes per lane, global -> LDS without staging registers; the wave writes LDS lane-linearly from `lds_dst` (wave-uniform)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, f16* lds_dst, unsigned voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)lds_dst, 16, voff, 0, 0, 0);
}
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* lds_dst, unsigned voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)lds_dst, 16, voff, 0, 0, 0);
}

// XCD-aware block order: blocks are dealt round-robin over the 8 XCDs, so XCD x gets the x-th contiguous eighth of a list of `nwg`
// entries.  Returns the list position of block `bid`; bijective for any nwg.
__device__ __forceinline__ int hd_xcd_contiguous(int bid, int nwg) {
  const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
  return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
}
