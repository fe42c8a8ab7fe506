// Batch assembly from an HBM-resident dataset (dataloader/cache.py): out[n] = f(arena[idx[n]]) for an arena of decoded uint8 images
// [S][C][H][W] and a device vector of N slot numbers, one launch per batch.  f is named by what the result must equal bit for bit:
//   HD_GATHER_U8           the bytes themselves (they go on to hd_augment_u8)
//   HD_GATHER_F32_DEFAULT  (float)b * fp32(1/255): what ATen computes for `u8.float().div_(255.0)` on the GPU (a Python-scalar divisor is
//                          inverted on the host in fp32 and multiplied)
//   HD_GATHER_F32_IEEE     (float)b / 255.0f, the correctly rounded quotient: ATen's `u8.float().div_(tensor(255.0))`
// The slot offset idx[n] * C*H*W is a 64-bit product: an LLVIP arena is 63 GB.  A slot number outside [0, S) -- the caller validates
// them on the host before the launch -- writes nothing rather than reading outside the arena.
// grid.y = image of the batch, grid.x = at most MAXBX blocks of AB lanes that walk the image with a grid-stride loop, so ONE pass covers
// MAXBX * AB * 16 = 1 MiB of an image on the 16-byte path (16 source bytes per lane and trip; a 3 x 512 x 640 image is 960 KiB) and
// MAXBX * AB = 64 Ki values on the byte path; larger images go round the loop again.  Every output element has one writer; no atomics,
// no workspace, no host synchronisation.
// The source rows are cold HBM by construction (an epoch touches every slot once) and nothing is read twice, so the caches only see a
// stream; every load and store instruction of a wave covers one contiguous run (kernels below).
#include "hd_block.h"
#pragma clang fp contract(off)

namespace {

constexpr int AB = 256;          // threads per block
constexpr int MAXBX = 256;       // most blocks per image (grid.x); grid.y = image of the batch

template <int MODE>
__device__ __forceinline__ float to_f32(uint32_t b) {
  return MODE == HD_GATHER_F32_IEEE ? (float)b / 255.0f : (float)b * (1.0f / 255.0f);
}

// u8 mode on the 16-byte path: `per` = C*H*W / 16 vectors per image, 16 bytes in and 16 bytes out per lane
__global__ __launch_bounds__(AB) void batch_gather_u8x16_kernel(const uint8_t* __restrict__ arena, int64_t S, const int64_t* __restrict__ idx,
                                                                int64_t per, uint8_t* __restrict__ out) {
  const int n = blockIdx.y;
  const int64_t slot = idx[n];
  if (slot < 0 || slot >= S) return;
  const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(arena + slot * per * 16);
  u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(out + (int64_t)n * per * 16);
  const int64_t step = (int64_t)gridDim.x * AB;
  for (int64_t g = (int64_t)blockIdx.x * AB + threadIdx.x; g < per; g += step) dst[g] = __builtin_nontemporal_load(src + g);
}

// float modes on the 16-byte path: `per` = C*H*W / 4 dwords per image.  A lane loads FOUR BYTES and stores ONE float4, four times per
// trip, AB dwords apart: every load instruction of a wave reads 256 consecutive bytes and every store instruction writes 1 KiB in a row
// (lane i at base + 16 i).  The first version had a lane load 16 bytes and store its four float4 itself, i.e. 64 pieces of 16 bytes at a
// 64-byte stride per store instruction: 14.9 us for 8 x 3 x 512 x 640 where a copy of the batch takes 10.2.
template <int MODE>
__global__ __launch_bounds__(AB) void batch_gather_f32x4_kernel(const uint8_t* __restrict__ arena, int64_t S, const int64_t* __restrict__ idx,
                                                                int64_t per, float* __restrict__ out) {
  const int n = blockIdx.y;
  const int64_t slot = idx[n];
  if (slot < 0 || slot >= S) return;
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(arena + slot * per * 4);
  f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(out + (int64_t)n * per * 4);
  constexpr int TILE = AB * 4;          // dwords per block and trip = the 4 KiB of the image a block of the u8 kernel moves
  const int64_t step = (int64_t)gridDim.x * TILE;
  for (int64_t base = (int64_t)blockIdx.x * TILE + threadIdx.x; base < per; base += step) {
    uint32_t q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + j * AB;
      q[j] = i < per ? __builtin_nontemporal_load(src + i) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + j * AB;
      if (i < per) {
        f32x4 v;
        v[0] = to_f32<MODE>(q[j] & 255u);
        v[1] = to_f32<MODE>((q[j] >> 8) & 255u);
        v[2] = to_f32<MODE>((q[j] >> 16) & 255u);
        v[3] = to_f32<MODE>(q[j] >> 24);
        dst[i] = v;
      }
    }
  }
}

// any other shape: one byte per lane
template <int MODE>
__global__ __launch_bounds__(AB) void batch_gather_byte_kernel(const uint8_t* __restrict__ arena, int64_t S, const int64_t* __restrict__ idx,
                                                               int64_t chw, void* __restrict__ out) {
  const int n = blockIdx.y;
  const int64_t slot = idx[n];
  if (slot < 0 || slot >= S) return;
  const uint8_t* __restrict__ src = arena + slot * chw;
  const int64_t step = (int64_t)gridDim.x * AB;
  for (int64_t g = (int64_t)blockIdx.x * AB + threadIdx.x; g < chw; g += step) {
    const uint32_t b = src[g];
    if (MODE == HD_GATHER_U8) (static_cast<uint8_t*>(out) + (int64_t)n * chw)[g] = (uint8_t)b;
    else (static_cast<float*>(out) + (int64_t)n * chw)[g] = to_f32<MODE>(b);
  }
}

inline dim3 grid_for(int64_t units, int N) {          // `units` of work per image, one per lane and trip
  const int64_t gx = (units + AB - 1) / AB;
  return dim3((unsigned)(gx > MAXBX ? MAXBX : gx), (unsigned)N);
}

template <int MODE>
void launch(bool vec, hipStream_t s, const uint8_t* arena, int64_t S, const int64_t* idx, int N, int64_t chw, void* out) {
  const dim3 block(AB);
  if (!vec)
    hipLaunchKernelGGL((batch_gather_byte_kernel<MODE>), grid_for(chw, N), block, 0, s, arena, S, idx, chw, out);
  else if constexpr (MODE == HD_GATHER_U8)
    hipLaunchKernelGGL(batch_gather_u8x16_kernel, grid_for(chw / 16, N), block, 0, s, arena, S, idx, chw / 16, static_cast<uint8_t*>(out));
  else
    hipLaunchKernelGGL((batch_gather_f32x4_kernel<MODE>), grid_for(chw / 16, N), block, 0, s, arena, S, idx, chw / 4, static_cast<float*>(out));
}

}  // namespace

extern "C" int hd_batch_gather_u8(const uint8_t* arena, int64_t S, const int64_t* idx, int N, int64_t chw, int mode, void* out, void* stream) {
  HD_CHECK_ARG(arena && idx && out, "hd_batch_gather_u8: null pointer (arena, idx and out are required)");
  HD_CHECK_ARG(S >= 1 && N >= 1 && N <= HD_GATHER_MAX_BATCH && chw >= 1,
               "hd_batch_gather_u8: need S >= 1, 1 <= N <= %d, C*H*W >= 1 (got S=%lld N=%d C*H*W=%lld)", HD_GATHER_MAX_BATCH, (long long)S, N,
               (long long)chw);
  HD_CHECK_ARG(mode == HD_GATHER_U8 || mode == HD_GATHER_F32_DEFAULT || mode == HD_GATHER_F32_IEEE,
               "hd_batch_gather_u8: mode must be HD_GATHER_U8, HD_GATHER_F32_DEFAULT or HD_GATHER_F32_IEEE (got %d)", mode);
  HD_CHECK_ARG(mode == HD_GATHER_U8 || (reinterpret_cast<uintptr_t>(out) & 3) == 0, "hd_batch_gather_u8: a float output must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  // the 16-byte path when every slot starts on a 16-byte boundary (C*H*W a multiple of 16 and both bases aligned); one byte per lane
  // otherwise: correct, not tuned
  const bool vec = chw % 16 == 0 && hd_aligned16(arena) && hd_aligned16(out);
  if (mode == HD_GATHER_U8) launch<HD_GATHER_U8>(vec, s, arena, S, idx, N, chw, out);
  else if (mode == HD_GATHER_F32_DEFAULT) launch<HD_GATHER_F32_DEFAULT>(vec, s, arena, S, idx, N, chw, out);
  else launch<HD_GATHER_F32_IEEE>(vec, s, arena, S, idx, N, chw, out);
  HD_CHECK_LAUNCH();
  return HD_OK;
}
