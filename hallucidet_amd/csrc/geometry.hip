// Paired geometric training augmentation (dataloader/geometry.py): horizontal flip and a box-safe crop, resized back to the input's
// shape, as ONE gather over a uint8 batch [N][C][H][W] (C = 1 or 3, every channel treated alike), from a dense batch or straight out of
// the dataset cache's arena [S][C][H][W] through N device slot numbers.
//
// Definition.  One record row per image: int32[8] = [flip, x0, y0, x1, y1, 0, 0, 0], 0 <= x0 < x1 <= W, 0 <= y0 < y1 <= H,
// cw = x1 - x0, ch = y1 - y0.  out = the bilinear resize (half-pixel centres, no antialias) of the crop window [x0, x1) x [y0, y1) of
// the horizontally flipped image (of the image itself when flip = 0) to H x W; cw <= W and ch <= H, so always a magnification.
//   position  integers: px = (2 ox + 1) cw - W, jx = floor(px / 2W) (towards -inf), rx = px - jx 2W; fx = fp32(rx) / fp32(2W), ONE IEEE
//             division of two exactly representable operands; xa = clamp(jx, 0, cw-1), xb = clamp(jx+1, 0, cw-1).  y alike with ch, H.
//   edges     taps are clamped to the crop (replicate), never read from outside it
//   column    crop column k is source column s = x0 + k, and W - 1 - s when flip
//   value     taps as fp32: t0 = v00 + fx (v01 - v00), t1 = v10 + fx (v11 - v10), v = t0 + fy (t1 - t0); every operation rounded once,
//             no fused multiply-add
//   byte      b = uint8(floor(v + 0.5f))
//   modes     HD_GEOM_U8: b;  HD_GEOM_F32_IEEE: fp32(b) / 255.0f, the correctly rounded quotient
// The record [0, 0, 0, W, H] gives jx = ox, fx = 0: the input bytes.
//
// Shape of the kernel.  W % 16 == 0 with 16-byte aligned bases: a block owns a tile of TR output rows x at most TC output columns of one
// plane.  It (1) copies the <= TR + 1 source rows the tile's taps touch, over the <= TC + 16 aligned source bytes they span, into LDS with
// 16-byte loads, (2) writes the column table (both tap offsets and fx per output column: the integer and the IEEE division are paid once
// per column of a tile, not once per pixel), the row table and, in f32 mode, the 256 quotients b / 255.0f (one IEEE division per thread
// and tile instead of one per value), (3) reads four taps per pixel from LDS and stores 16 bytes per lane: 16 pixels in u8 mode, a
// float4 in f32 mode.  A tile as wide as the image is one contiguous piece of the output and is walked flat, so
// every store instruction of a wave covers one contiguous run (1 KiB); in a narrower tile (W > TC) the vectors of a row are padded to
// whole waves, so a wave never straddles two rows.  The source bytes are read from memory once per tile ((TR + 1) / TR of the image at
// most); the 4 taps per pixel come from LDS.  Staging through LDS instead of reading taps from global memory was chosen because the tap
// addresses of a wave are unaligned single bytes: as global loads they are four byte-loads per pixel through the texture path for one
// byte stored, as LDS reads the global side is as wide and as contiguous as hd_batch_gather_u8's.  In u8 mode lanes are 16 source bytes
// apart and the tap reads meet 4-way bank conflicts; the f32 mode, the one the prefetcher uses, has lanes 4 bytes apart and none.
// Any other shape: one value per lane straight from global memory: correct, not tuned.
// One writer per output element, no atomics, no workspace, no host synchronisation; a slot outside [0, S) writes nothing.  Every index
// derived from a record is clamped to H and W first: no row content reads outside src or writes outside out.
#include "hd_block.h"
#pragma clang fp contract(off)

namespace {

constexpr int GB = 256;                  // threads per block (thread t writes the quotient t / 255.0f of a tile)
static_assert(GB == 256, "one thread per byte value");
constexpr int TR = 8;                    // output rows of a tile
constexpr int TC = 1024;                 // most output columns of a tile
constexpr int SPAN = TC + 32;            // staged bytes per source row: TC + 1 tap columns, cut out in whole 16-byte pieces
constexpr int SROWS = TR + 1;            // source rows of a tile: a magnification advances at most one source row per output row

struct Rec {
  int flip, x0, y0, cw, ch;
};

// the record of image n with every field forced into the extents of the call
__device__ __forceinline__ Rec load_rec(const int* __restrict__ rows, int n, int H, int W) {
  const int* p = rows + (size_t)n * HD_GEOM_ROW;
  Rec r;
  r.flip = p[0] != 0;
  r.x0 = min(max(p[1], 0), W - 1);
  r.y0 = min(max(p[2], 0), H - 1);
  r.cw = min(max(p[3], r.x0 + 1), W) - r.x0;
  r.ch = min(max(p[4], r.y0 + 1), H) - r.y0;
  return r;
}

// output coordinate o of an axis of extent E whose crop has c samples -> taps a, b in [0, c) and the weight f of b
__device__ __forceinline__ void position(int o, int c, int E, int& a, int& b, float& f) {
  const int p = (2 * o + 1) * c - E, d = 2 * E;
  const int j = p >= 0 ? p / d : -((d - 1 - p) / d);
  f = (float)(p - j * d) / (float)d;
  a = min(max(j, 0), c - 1);
  b = min(max(j + 1, 0), c - 1);
}

// the taps alone (the extents of a tile need no weight)
__device__ __forceinline__ void taps(int o, int c, int E, int& a, int& b) {
  const int p = (2 * o + 1) * c - E, d = 2 * E;
  const int j = p >= 0 ? p / d : -((d - 1 - p) / d);
  a = min(max(j, 0), c - 1);
  b = min(max(j + 1, 0), c - 1);
}

__device__ __forceinline__ int src_col(const Rec& r, int k, int W) { return r.flip ? W - 1 - (r.x0 + k) : r.x0 + k; }

__device__ __forceinline__ uint32_t blend(uint32_t b00, uint32_t b01, uint32_t b10, uint32_t b11, float fx, float fy) {
  const float v00 = (float)b00, v01 = (float)b01, v10 = (float)b10, v11 = (float)b11;
  const float t0 = v00 + fx * (v01 - v00);
  const float t1 = v10 + fx * (v11 - v10);
  const float v = t0 + fy * (t1 - t0);
  return min((uint32_t)floorf(v + 0.5f), 255u);
}

template <int MODE>
__global__ __launch_bounds__(GB) void geometry_wide_kernel(const uint8_t* __restrict__ src, int64_t S, const int64_t* __restrict__ idx,
                                                           const int* __restrict__ rows, int C, int H, int W, int nchunk,
                                                           void* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t srow[SROWS * SPAN];
  __shared__ uint2 xtab[TC];             // .x = offset of tap a | offset of tap b << 16 (bytes into a staged row), .y = bits of fx
  __shared__ int ya[TR], yb[TR];         // byte offsets of the two staged rows of an output row
  __shared__ float yf[TR];
  __shared__ float q255[MODE == HD_GEOM_U8 ? 1 : 256];      // b / 255.0f for every byte: one IEEE division per thread and tile, not per value
  const int tid = threadIdx.x, n = blockIdx.y, c = blockIdx.z;
  const Rec r = load_rec(rows, n, H, W);                   // before the slot test: the two loads do not wait for each other
  const int64_t slot = idx ? idx[n] : (int64_t)n;
  if (slot < 0 || slot >= S) return;
  if constexpr (MODE != HD_GEOM_U8) q255[tid] = (float)tid / 255.0f;
  const int chunk = blockIdx.x % nchunk, rt = blockIdx.x / nchunk;
  const int ox0 = chunk * TC, tw = min(TC, W - ox0);
  const int oy0 = rt * TR, th = min(TR, H - oy0);

  int a, b;
  float f;
  taps(ox0, r.cw, W, a, b);
  const int cLo = a;
  taps(ox0 + tw - 1, r.cw, W, a, b);
  const int cHi = b;
  const int sLo = r.flip ? src_col(r, cHi, W) : src_col(r, cLo, W);
  const int sHi = r.flip ? src_col(r, cLo, W) : src_col(r, cHi, W);
  const int aLo = sLo & ~15;
  const int nvec = min((sHi - aLo) / 16 + 1, SPAN / 16);
  taps(oy0, r.ch, H, a, b);
  const int kLo = a;
  taps(oy0 + th - 1, r.ch, H, a, b);
  const int nrows = min(b - kLo + 1, SROWS);

  const uint8_t* __restrict__ plane = src + (slot * C + c) * ((int64_t)H * W);
  for (int v = tid; v < nrows * nvec; v += GB) {
    const int rr = v / nvec, cc = v - rr * nvec;
    *reinterpret_cast<u32x4*>(srow + rr * SPAN + cc * 16) =
        *reinterpret_cast<const u32x4*>(plane + (int64_t)(r.y0 + kLo + rr) * W + aLo + cc * 16);
  }
  const int lastb = nvec * 16 - 1;
  for (int i = tid; i < tw; i += GB) {
    position(ox0 + i, r.cw, W, a, b, f);
    const int oa = min(max(src_col(r, a, W) - aLo, 0), lastb), ob = min(max(src_col(r, b, W) - aLo, 0), lastb);
    xtab[i] = make_uint2((uint32_t)oa | ((uint32_t)ob << 16), __float_as_uint(f));
  }
  if (tid < th) {
    position(oy0 + tid, r.ch, H, a, b, f);
    ya[tid] = min(max(a - kLo, 0), nrows - 1) * SPAN;
    yb[tid] = min(max(b - kLo, 0), nrows - 1) * SPAN;
    yf[tid] = f;
  }
  __syncthreads();

  constexpr int V = MODE == HD_GEOM_U8 ? 16 : 4;         // pixels per lane and store
  const int rv = tw / V;                                 // vectors per tile row
  const int rvp = nchunk == 1 ? rv : (rv + 63) & ~63;    // a tile narrower than the image: whole waves per row
  const int64_t obase = (((int64_t)n * C + c) * H + oy0) * W + ox0;
  for (int q = tid; q < th * rvp; q += GB) {
    const int row = q / rvp, cv = q - row * rvp;
    if (cv >= rv) continue;
    const uint8_t* ra = srow + ya[row];
    const uint8_t* rb = srow + yb[row];
    const float fy = yf[row];
    uint32_t px[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const uint2 t = xtab[cv * V + i];
      const uint32_t oa = t.x & 0xffffu, ob = t.x >> 16;
      px[i] = blend(ra[oa], ra[ob], rb[oa], rb[ob], __uint_as_float(t.y), fy);
    }
    const int64_t o = obase + (int64_t)row * W + cv * V;
    if constexpr (MODE == HD_GEOM_U8) {
      u32x4 w;
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | (px[4 * k + 3] << 24);
      *reinterpret_cast<u32x4*>(static_cast<uint8_t*>(out) + o) = w;
    } else {
      f32x4 w;
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = q255[px[k]];
      *reinterpret_cast<f32x4*>(static_cast<float*>(out) + o) = w;
    }
  }
}

// any other shape: one value per lane, taps straight from global memory
template <int MODE>
__global__ __launch_bounds__(GB) void geometry_byte_kernel(const uint8_t* __restrict__ src, int64_t S, const int64_t* __restrict__ idx,
                                                           const int* __restrict__ rows, int C, int H, int W, void* __restrict__ out) {
  const int n = blockIdx.y, c = blockIdx.z;
  const int64_t slot = idx ? idx[n] : (int64_t)n;
  if (slot < 0 || slot >= S) return;
  const int hw = H * W;
  const int g = blockIdx.x * GB + threadIdx.x;
  if (g >= hw) return;
  const Rec r = load_rec(rows, n, H, W);
  const int oy = g / W, ox = g - oy * W;
  int xa, xb, ya, yb;
  float fx, fy;
  position(ox, r.cw, W, xa, xb, fx);
  position(oy, r.ch, H, ya, yb, fy);
  const uint8_t* __restrict__ plane = src + (slot * C + c) * (int64_t)hw;
  const uint8_t* ra = plane + (int64_t)(r.y0 + ya) * W;
  const uint8_t* rb = plane + (int64_t)(r.y0 + yb) * W;
  const int sa = src_col(r, xa, W), sb = src_col(r, xb, W);
  const uint32_t bv = blend(ra[sa], ra[sb], rb[sa], rb[sb], fx, fy);
  const int64_t o = ((int64_t)n * C + c) * hw + g;
  if (MODE == HD_GEOM_U8) static_cast<uint8_t*>(out)[o] = (uint8_t)bv;
  else static_cast<float*>(out)[o] = (float)bv / 255.0f;
}

template <int MODE>
void launch(bool wide, hipStream_t s, const uint8_t* src, int64_t S, const int64_t* idx, const int* rows, int N, int C, int H, int W, void* out) {
  if (wide) {
    const int nchunk = (W + TC - 1) / TC, ntile = (H + TR - 1) / TR;
    hipLaunchKernelGGL((geometry_wide_kernel<MODE>), dim3((unsigned)(nchunk * ntile), (unsigned)N, (unsigned)C), dim3(GB), 0, s, src, S, idx,
                       rows, C, H, W, nchunk, out);
  } else {
    hipLaunchKernelGGL((geometry_byte_kernel<MODE>), dim3((unsigned)((H * W + GB - 1) / GB), (unsigned)N, (unsigned)C), dim3(GB), 0, s, src, S,
                       idx, rows, C, H, W, out);
  }
}

}  // namespace

extern "C" int hd_geometry_check_rows(const int32_t* rows, int N, int H, int W) {
  HD_CHECK_ARG(rows, "hd_geometry_check_rows: null pointer");
  HD_CHECK_ARG(N >= 1 && N <= HD_GEOM_MAX_BATCH && H >= 2 && W >= 2 && H <= HD_GEOM_MAX_EXTENT && W <= HD_GEOM_MAX_EXTENT,
               "hd_geometry_check_rows: need 1 <= N <= %d, 2 <= H, W <= %d (got N=%d H=%d W=%d)", HD_GEOM_MAX_BATCH, HD_GEOM_MAX_EXTENT, N, H, W);
  for (int n = 0; n < N; ++n) {
    const int32_t* p = rows + (size_t)n * HD_GEOM_ROW;
    HD_CHECK_ARG((p[0] == 0 || p[0] == 1) && 0 <= p[1] && p[1] < p[3] && p[3] <= W && 0 <= p[2] && p[2] < p[4] && p[4] <= H,
                 "hd_geometry_check_rows: row %d = [%d, %d, %d, %d, %d]: need flip in {0, 1}, 0 <= x0 < x1 <= %d, 0 <= y0 < y1 <= %d", n, p[0],
                 p[1], p[2], p[3], p[4], W, H);
    HD_CHECK_ARG(p[5] == 0 && p[6] == 0 && p[7] == 0, "hd_geometry_check_rows: row %d: the three reserved fields must be 0", n);
  }
  return HD_OK;
}

extern "C" int hd_geometry_u8(const uint8_t* src, int64_t S, const int64_t* idx, const int32_t* rows, int N, int C, int H, int W, int mode,
                              void* out, void* stream) {
  HD_CHECK_ARG(src && rows && out, "hd_geometry_u8: null pointer (src, rows and out are required)");
  HD_CHECK_ARG(N >= 1 && N <= HD_GEOM_MAX_BATCH && (C == 1 || C == 3) && H >= 2 && W >= 2 && H <= HD_GEOM_MAX_EXTENT && W <= HD_GEOM_MAX_EXTENT,
               "hd_geometry_u8: need 1 <= N <= %d, C in (1, 3), 2 <= H, W <= %d (got N=%d C=%d H=%d W=%d)", HD_GEOM_MAX_BATCH,
               HD_GEOM_MAX_EXTENT, N, C, H, W);
  HD_CHECK_ARG(idx ? S >= 1 : S == N, "hd_geometry_u8: an arena needs S >= 1 slots, a dense batch (idx = NULL) S == N (got S=%lld N=%d)",
               (long long)S, N);
  HD_CHECK_ARG(mode == HD_GEOM_U8 || mode == HD_GEOM_F32_IEEE, "hd_geometry_u8: mode must be HD_GEOM_U8 or HD_GEOM_F32_IEEE (got %d)", mode);
  HD_CHECK_ARG(mode == HD_GEOM_U8 || (reinterpret_cast<uintptr_t>(out) & 3) == 0, "hd_geometry_u8: a float output must be 4-byte aligned");
  HD_CHECK_ARG((reinterpret_cast<uintptr_t>(rows) & 3) == 0, "hd_geometry_u8: rows must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const bool wide = W % 16 == 0 && hd_aligned16(src) && hd_aligned16(out);
  if (mode == HD_GEOM_U8) launch<HD_GEOM_U8>(wide, s, src, S, idx, rows, N, C, H, W, out);
  else launch<HD_GEOM_F32_IEEE>(wide, s, src, S, idx, rows, N, C, H, W, out);
  HD_CHECK_LAUNCH();
  return HD_OK;
}
