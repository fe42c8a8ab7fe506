// Wave (64 lanes) and block primitives of the bandwidth-bound and selection kernels: reductions, scans, ordered compaction ranks,
// the order-preserving float <-> uint32 key map, and 16-byte plane access.  One definition each, so that a fix to one of them reaches
// every kernel that uses it.  Blocks are whole waves (blockDim.x a multiple of 64, one-dimensional); LDS scratch is the caller's.
// Nothing here depends on `f16`: the files built twice (-DHD_STORE_F32) get the same code in both builds.
// Not for the partial-wave, channel-interleaved reductions of the convolution / BatchNorm kernels: their strides and LDS layouts are
// their own (elementwise.hip, conv_epilogue.h, conv_f32.hip, conv3x3_c32to128.hip, conv3x3_small.hip, wgrad.hip).
#pragma once
#include "hd_common.h"

// ---- combining functors ----------------------------------------------------------------------------------------------------
struct HdSum {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct HdMax {
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
};
struct HdMin {
  __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
  __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
};

// ---- wave reduce: xor butterfly 32 .. 1, every lane ends with the wave's result ----------------------------------------------
template <class T, class F>
__device__ __forceinline__ T hd_wave_reduce(T v, F f) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = f(v, __shfl_xor(v, d));
  return v;
}
// two values, each with its own type and functor (max + count, min + max, two sums), both advanced at every step
template <class TA, class FA, class TB, class FB>
__device__ __forceinline__ void hd_wave_reduce2(TA& a, FA fa, TB& b, FB fb) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a = fa(a, __shfl_xor(a, d));
    b = fb(b, __shfl_xor(b, d));
  }
}
// N values of one type, all of them advanced at every step
template <int N, class T, class F>
__device__ __forceinline__ void hd_wave_reduce(T (&v)[N], F f) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = f(v[k], __shfl_xor(v[k], d));
}

// ---- block reduce ----------------------------------------------------------------------------------------------------------------
// Lane 0 of wave w stores the wave-reduced v[k] to sm[w * N + k]; ONE barrier; on return every thread may read the partials.  The fold
// over them belongs to the caller where its order is not the left fold below (a pairwise tree, thread 0 only).  sm is reusable after
// the caller's next barrier.
template <int N, class T>
__device__ __forceinline__ void hd_block_put(const T (&v)[N], T* sm) {
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) sm[w * N + k] = v[k];
  }
  __syncthreads();
}
// every thread: v[k] = (..(p[0][k] . p[1][k]) . ..) . p[WAVES-1][k], the partials folded left to right
template <int WAVES, int N, class T, class F>
__device__ __forceinline__ void hd_block_fold(T (&v)[N], F f, const T* sm) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    T r = sm[k];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = f(r, sm[w * N + k]);
    v[k] = r;
  }
}
template <int WAVES, int N, class T, class F>
__device__ __forceinline__ void hd_block_reduce(T (&v)[N], F f, T* sm) {
  hd_wave_reduce(v, f);
  hd_block_put(v, sm);
  hd_block_fold<WAVES>(v, f, sm);
}
// one value: partial of wave w at sm[w]
template <class T>
__device__ __forceinline__ void hd_block_put(T v, T* sm) {
  const T v1[1] = {v};
  hd_block_put(v1, sm);
}
template <int WAVES, class T, class F>
__device__ __forceinline__ T hd_block_reduce(T v, F f, T* sm) {
  T v1[1] = {v};
  hd_block_reduce<WAVES>(v1, f, sm);
  return v1[0];
}
// the two-stage deterministic sum of the loss kernels: sm holds 2 * WAVES floats
template <int WAVES>
__device__ __forceinline__ void hd_block_sum2(float& a, float& b, float* sm) {
  float v[2] = {a, b};
  hd_block_reduce<WAVES>(v, HdSum(), sm);
  a = v[0];
  b = v[1];
}

// ---- scans -------------------------------------------------------------------------------------------------------------------------
// inclusive scan over the wave's lanes; `lane` = the caller's lane index
template <class T>
__device__ __forceinline__ T hd_wave_scan(T v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}
// inclusive scan over the block's threads, the block total in *tot; sm holds WAVES values.  Two barriers: sm is free on return.
template <int WAVES, class T>
__device__ __forceinline__ T hd_block_scan(T v, T* sm, T* tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = hd_wave_scan(v, lane);
  if (lane == 63) sm[w] = v;
  __syncthreads();
  T off = 0, all = 0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) {
    const T s = sm[i];
    off += i < w ? s : 0;
    all += s;
  }
  __syncthreads();
  *tot = all;
  return v + off;
}

// ---- ordered compaction -------------------------------------------------------------------------------------------------------------
// single wave: rank of `lane` among the flagged lanes of bal = __ballot(flag), in lane order; their number is __popcll(bal)
__device__ __forceinline__ int hd_ballot_rank(uint64_t bal, int lane) { return __popcll(bal & ((1ull << lane) - 1ull)); }
// rank of this thread among the flagged threads of the block, in thread order; *total = their number.  wcnt holds WAVES ints.
// ONE barrier, between the write of wcnt and its reads: a caller that calls again (a chunked loop) puts a barrier of its own between
// two calls -- after its use of the rank, or in front of the call.
template <int WAVES>
__device__ __forceinline__ int hd_block_rank(bool flag, int* wcnt, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t bal = __ballot(flag);
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int off = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) off += wcnt[w];
    all += wcnt[w];
  }
  *total = all;
  return off + hd_ballot_rank(bal, lane);
}

// ---- order-preserving map float -> uint32 and back: a < b <=> key(a) < key(b) on the float bits (-0 below +0, NaNs at the ends) ----
__device__ __forceinline__ uint32_t hd_float_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float hd_key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- V consecutive floats of one plane: one 16-byte load / store (V = 4, p 16-byte aligned) or one scalar (V = 1) --------------------
template <int V>
__device__ __forceinline__ void hd_ldv(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void hd_stv(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    f32x4 t;
    t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = v[0];
  }
}
// host: may p be accessed 16 bytes at a time (an absent, null, operand does not stand in the way)
static inline bool hd_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
