// Photometric training augmentation of the reference's detector recipe (train_detector.py:401-410: ColorJitter, RandomInvert,
// RandomAdjustSharpness, RandomEqualize on the decoded PIL image) on the uint8 batch in HBM, bit for bit what Pillow computes.
// Images are planar uint8 [N][C][H][W], C = 3 (RGB) or 1 (PIL mode L); one parameter row of HD_AUG_ROW floats per image, read on
// the device, says which operations run and in which order, so the launch sequence is the same for every batch:
//   memset  the integer accumulators (L sums, histograms)
//   pass A  sum of L over the state the contrast operation sees (the jitter operations drawn before it applied on the fly)
//   pass B  every jitter operation in the drawn order + invert, x -> out (or -> tmp when sharpness follows); histograms when
//           equalize follows directly
//   pass C  sharpness, tmp -> out, histograms when equalize follows; images without sharpness leave at once
//   pass D  equalize in place on out; images without it leave at once
// Whole-image quantities are 32-bit integer accumulators (registers -> wave -> LDS -> one global atomic per block and bin): the
// result does not depend on the order of arrival.  255 * H*W must fit in 32 bits: H*W <= HD_AUG_MAX_PIXELS.
// Float steps follow Pillow's C code operation by operation: every product and sum below is one rounding (no contraction), the
// quotients are correctly rounded, and the doubles of the hue conversion are doubles.
#include "hd_block.h"
#pragma clang fp contract(off)

namespace {

constexpr int AB = 256;          // threads per block
constexpr int MAXBX = 128;       // most blocks per image (grid.x); grid.y = image

enum { OP_BRIGHT = 0, OP_CONTRAST = 1, OP_SAT = 2, OP_HUE = 3, OP_NONE = 15 };

struct Row {
  int ord;                       // four operation codes, 4 bits each, first operation in the low bits
  float fb, fc, fs, fsharp;
  int shift;
  bool invert, sharp, equalize, has_contrast;
};

__device__ __forceinline__ Row load_row(const float* __restrict__ params, int n) {
  const float* p = params + (size_t)n * HD_AUG_ROW;
  Row r;
  r.ord = 0;
  r.has_contrast = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int op = (int)p[j];
    r.ord |= ((op >= 0 && op <= 3) ? op : OP_NONE) << (4 * j);
    r.has_contrast = r.has_contrast || op == OP_CONTRAST;
  }
  r.fb = p[4];
  r.fc = p[5];
  r.fs = p[6];
  r.shift = (int)((double)p[7] * 255.0);      // torchvision: uint8(hue_factor * 255), the product in double
  r.invert = p[8] != 0.f;
  r.sharp = p[9] != 0.f;
  r.equalize = p[10] != 0.f;
  r.fsharp = p[11];
  return r;
}

__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ImagingBlend: temp = in1 + alpha * (in2 - in1) in float; alpha in [0, 1]: truncate, else clip then truncate
__device__ __forceinline__ int blend(int d, int x, float a) {
  const float prod = a * (float)(x - d);
  const float t = (float)d + prod;
  if (a >= 0.f && a <= 1.f) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Pillow Convert.c rgb2hsv / hsv2rgb followed operation by operation (float quotients, the two long hue branches in double)
__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int uh = 0, us = 0;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx) h = bc - gc;
    else if (g == mx) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    double hd = (double)h / 6.0 + 1.0;         // in [5/6, 11/6]: fmod(hd, 1.0) is hd or hd - 1, both exact
    if (hd >= 1.0) hd = hd - 1.0;
    h = (float)hd;
    uh = clip255((int)((double)h * 255.0));
    us = clip255((int)((double)s * 255.0));
  }
  uh = (uh + shift) & 255;
  if (us == 0) {
    r = g = b = mx;
    return;
  }
  const float fs = (float)((double)us / 255.0);
  const float hh = (float)(((double)uh * 6.0) / 255.0);
  const int i = (int)floorf(hh);
  const float f = hh - (float)i;
  const float vf = (float)mx;
  const float one_fs = 1.f - fs;
  const float pf = vf * one_fs;
  const float fsf = fs * f;
  const float one_fsf = 1.f - fsf;
  const float qf = vf * one_fsf;
  const float one_f = 1.f - f;
  const float fs1f = fs * one_f;
  const float one_fs1f = 1.f - fs1f;
  const float tf = vf * one_fs1f;
  const int p = clip255((int)floor((double)pf + 0.5));
  const int q = clip255((int)floor((double)qf + 0.5));
  const int t = clip255((int)floor((double)tf + 0.5));
  const int v = mx;
  switch (i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// the jitter operations of one row, in its order, on V pixels held as v[channel][pixel]; m = the contrast mean.  With
// until_contrast the walk ends in front of the contrast operation (the state its mean is taken of).
template <int C, int V>
__device__ __forceinline__ void jitter(const Row& row, int m, bool until_contrast, int (&v)[C][V]) {
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    const int op = (row.ord >> (4 * j)) & 15;
    if (op == OP_BRIGHT) {
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < V; ++k) v[c][k] = blend(0, v[c][k], row.fb);
    } else if (op == OP_CONTRAST) {
      if (until_contrast) break;
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < V; ++k) v[c][k] = blend(m, v[c][k], row.fc);
    } else if (C == 3 && op == OP_SAT) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int l = luma(v[0][k], v[C > 1 ? 1 : 0][k], v[C > 2 ? 2 : 0][k]);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][k] = blend(l, v[c][k], row.fs);
      }
    } else if (C == 3 && op == OP_HUE) {
#pragma unroll
      for (int k = 0; k < V; ++k) hue_shift(v[0][k], v[C > 1 ? 1 : 0][k], v[C > 2 ? 2 : 0][k], row.shift);
    }
  }
}

// V consecutive bytes of one plane: one 16-byte access (V = 16) or one byte (V = 1)
template <int V>
__device__ __forceinline__ void ld_bytes(const uint8_t* __restrict__ p, int (&v)[V]) {
  if constexpr (V == 16) {
    const u32x4 t = *reinterpret_cast<const u32x4*>(p);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = (int)((w[k >> 2] >> ((k & 3) * 8)) & 255u);
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void st_bytes(uint8_t* __restrict__ p, const int (&v)[V]) {
  if constexpr (V == 16) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)v[k] << ((k & 3) * 8);
    u32x4 t;
    t.x = w[0]; t.y = w[1]; t.z = w[2]; t.w = w[3];
    *reinterpret_cast<u32x4*>(p) = t;
  } else {
    *p = (uint8_t)v[0];
  }
}

template <int C>
__device__ __forceinline__ void hist_clear(uint32_t* sh) {
  for (int i = threadIdx.x; i < C * 256; i += AB) sh[i] = 0u;
  __syncthreads();
}
template <int C>
__device__ __forceinline__ void hist_flush(const uint32_t* sh, uint32_t* __restrict__ gh) {
  __syncthreads();
  for (int i = threadIdx.x; i < C * 256; i += AB) {
    const uint32_t v = sh[i];
    if (v) atomicAdd(gh + i, v);
  }
}

// ---- pass A: sums[n] = sum of L over the state contrast sees
template <int C, int V>
__global__ __launch_bounds__(AB) void aug_sum_kernel(const uint8_t* __restrict__ x, const float* __restrict__ params, int P,
                                                      uint32_t* __restrict__ sums) {
  const int n = blockIdx.y;
  const Row row = load_row(params, n);
  if (!row.has_contrast) return;
  __shared__ uint32_t sm[AB / 64];
  const uint8_t* xi = x + (size_t)n * C * P;
  uint32_t acc = 0u;
  const int groups = P / V;
  for (int gidx = blockIdx.x * AB + threadIdx.x; gidx < groups; gidx += gridDim.x * AB) {
    int v[C][V];
#pragma unroll
    for (int c = 0; c < C; ++c) ld_bytes<V>(xi + (size_t)c * P + (size_t)gidx * V, v[c]);
    jitter<C, V>(row, 0, true, v);
#pragma unroll
    for (int k = 0; k < V; ++k) acc += (uint32_t)(C == 3 ? luma(v[0][k], v[C > 1 ? 1 : 0][k], v[C > 2 ? 2 : 0][k]) : v[0][k]);
  }
  hd_block_put(hd_wave_reduce(acc, HdSum()), sm);
  if (threadIdx.x == 0) {
    uint32_t t = 0u;
#pragma unroll
    for (int w = 0; w < AB / 64; ++w) t += sm[w];
    atomicAdd(sums + n, t);
  }
}

// ---- pass B: the jitter operations in the drawn order, then invert
template <int C, int V>
__global__ __launch_bounds__(AB) void aug_point_kernel(const uint8_t* __restrict__ x, const float* __restrict__ params, int P,
                                                        const uint32_t* __restrict__ sums, uint8_t* __restrict__ out,
                                                        uint8_t* __restrict__ tmp, uint32_t* __restrict__ hist) {
  const int n = blockIdx.y;
  const Row row = load_row(params, n);
  __shared__ uint32_t sh[C * 256];
  const bool do_hist = row.equalize && !row.sharp;
  if (do_hist) hist_clear<C>(sh);
  int m = 0;
  if (row.has_contrast) m = (int)((double)sums[n] / (double)P + 0.5);
  const uint8_t* xi = x + (size_t)n * C * P;
  uint8_t* yi = (row.sharp ? tmp : out) + (size_t)n * C * P;
  const int groups = P / V;
  for (int gidx = blockIdx.x * AB + threadIdx.x; gidx < groups; gidx += gridDim.x * AB) {
    int v[C][V];
#pragma unroll
    for (int c = 0; c < C; ++c) ld_bytes<V>(xi + (size_t)c * P + (size_t)gidx * V, v[c]);
    jitter<C, V>(row, m, false, v);
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (row.invert) v[c][k] = 255 - v[c][k];
        if (do_hist) atomicAdd(&sh[c * 256 + v[c][k]], 1u);
      }
      st_bytes<V>(yi + (size_t)c * P + (size_t)gidx * V, v[c]);
    }
  }
  if (do_hist) hist_flush<C>(sh, hist + (size_t)n * C * 256);
}

// ---- pass C: sharpness = blend(SMOOTH(x), x, f), SMOOTH = [1 1 1; 1 5 1; 1 1 1] / 13 with the border copied
template <int C, int V>
__global__ __launch_bounds__(AB) void aug_sharp_kernel(const uint8_t* __restrict__ tmp, const float* __restrict__ params, int H, int W,
                                                        uint8_t* __restrict__ out, uint32_t* __restrict__ hist) {
  const int n = blockIdx.y;
  const Row row = load_row(params, n);
  if (!row.sharp) return;
  __shared__ uint32_t sh[C * 256];
  if (row.equalize) hist_clear<C>(sh);
  const int P = H * W;
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  const int groups = P / V;
  for (int gidx = blockIdx.x * AB + threadIdx.x; gidx < groups; gidx += gridDim.x * AB) {
    const int p0 = gidx * V;                 // V == 16 only with W % 16 == 0: the group lies in one row
    const int y = p0 / W, x0 = p0 - y * W;
    const bool inner_row = y > 0 && y < H - 1;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const uint8_t* pl = tmp + ((size_t)n * C + c) * P;
      int mid[V], res[V];
      ld_bytes<V>(pl + p0, mid);
      if (inner_row) {
        int up[V], dn[V];
        ld_bytes<V>(pl + p0 - W, up);
        ld_bytes<V>(pl + p0 + W, dn);
        // columns x0 - 1 and x0 + V of the three rows (absent at the image border, where the pixel is copied)
        int l3[3] = {0, 0, 0}, r3[3] = {0, 0, 0};
        if (x0 > 0) {
          l3[0] = pl[p0 - W - 1]; l3[1] = pl[p0 - 1]; l3[2] = pl[p0 + W - 1];
        }
        if (x0 + V < W) {
          r3[0] = pl[p0 - W + V]; r3[1] = pl[p0 + V]; r3[2] = pl[p0 + W + V];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int xx = x0 + k;
          const int a0 = k > 0 ? up[k > 0 ? k - 1 : 0] : l3[0], a2 = k < V - 1 ? up[k < V - 1 ? k + 1 : 0] : r3[0];
          const int b0 = k > 0 ? mid[k > 0 ? k - 1 : 0] : l3[1], b2 = k < V - 1 ? mid[k < V - 1 ? k + 1 : 0] : r3[1];
          const int c0 = k > 0 ? dn[k > 0 ? k - 1 : 0] : l3[2], c2 = k < V - 1 ? dn[k < V - 1 ? k + 1 : 0] : r3[2];
          float acc = (float)a0 * k1;          // row-major taps, each product rounded, then each sum
          float t;
          t = (float)up[k] * k1;  acc = acc + t;
          t = (float)a2 * k1;     acc = acc + t;
          t = (float)b0 * k1;     acc = acc + t;
          t = (float)mid[k] * k5; acc = acc + t;
          t = (float)b2 * k1;     acc = acc + t;
          t = (float)c0 * k1;     acc = acc + t;
          t = (float)dn[k] * k1;  acc = acc + t;
          t = (float)c2 * k1;     acc = acc + t;
          acc = acc + 0.5f;
          const int sm = acc <= 0.f ? 0 : (acc >= 255.f ? 255 : (int)acc);
          res[k] = (xx == 0 || xx == W - 1) ? mid[k] : blend(sm, mid[k], row.fsharp);
        }
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) res[k] = mid[k];
      }
      if (row.equalize) {
#pragma unroll
        for (int k = 0; k < V; ++k) atomicAdd(&sh[c * 256 + res[k]], 1u);
      }
      st_bytes<V>(out + ((size_t)n * C + c) * P + p0, res);
    }
  }
  if (row.equalize) hist_flush<C>(sh, hist + (size_t)n * C * 256);
}

// ---- pass D: ImageOps.equalize per channel, in place
template <int C, int V>
__global__ __launch_bounds__(AB) void aug_equalize_kernel(uint8_t* __restrict__ out, const float* __restrict__ params, int P,
                                                           const uint32_t* __restrict__ hist) {
  static_assert(AB == 256, "one thread per histogram bin");
  const int n = blockIdx.y;
  const Row row = load_row(params, n);
  if (!row.equalize) return;
  __shared__ uint32_t scan[256];
  __shared__ int red[2][AB / 64];
  __shared__ uint8_t lut[C * 256];
  const int i = threadIdx.x;
  for (int c = 0; c < C; ++c) {
    const uint32_t h = hist[((size_t)n * C + c) * 256 + i];
    // inclusive scan of the 256 bins
    scan[i] = h;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const uint32_t add = i >= d ? scan[i - d] : 0u;
      __syncthreads();
      scan[i] += add;
      __syncthreads();
    }
    // last non-empty bin and number of non-empty bins
    int last = h ? i : -1, cnt = h ? 1 : 0;
    hd_wave_reduce2(last, HdMax(), cnt, HdSum());
    if ((i & 63) == 0) {
      red[0][i >> 6] = last;
      red[1][i >> 6] = cnt;
    }
    __syncthreads();
    last = max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3]));
    cnt = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    int v = i;
    if (cnt > 1) {
      const uint32_t h_last = scan[last] - (last > 0 ? scan[last - 1] : 0u);
      const uint32_t step = ((uint32_t)P - h_last) / 255u;
      if (step != 0u) {
        const uint32_t q = (step / 2u + (scan[i] - h)) / step;
        v = q > 255u ? 255 : (int)q;
      }
    }
    lut[c * 256 + i] = (uint8_t)v;
    __syncthreads();
  }
  uint8_t* yi = out + (size_t)n * C * P;
  const int groups = P / V;
  for (int gidx = blockIdx.x * AB + threadIdx.x; gidx < groups; gidx += gridDim.x * AB) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      uint8_t* p = yi + (size_t)c * P + (size_t)gidx * V;
      int v[V];
      ld_bytes<V>(p, v);
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = lut[c * 256 + v[k]];
      st_bytes<V>(p, v);
    }
  }
}

inline dim3 grid_for(int P, int V, int N) {
  int gx = hd_cdiv(P / V, AB);
  return dim3(gx > MAXBX ? MAXBX : gx, N);
}

// VP: bytes per lane of the three pointwise passes (they walk the flat plane), VS: of the sharpness pass (it needs whole rows)
template <int C, int VP, int VS>
void launch_all(hipStream_t s, const uint8_t* x, const float* params, int N, int H, int W, uint8_t* out, uint8_t* tmp, uint32_t* sums,
                uint32_t* hist) {
  const int P = H * W;
  const dim3 gp = grid_for(P, VP, N), gs = grid_for(P, VS, N), block(AB);
  hipLaunchKernelGGL((aug_sum_kernel<C, VP>), gp, block, 0, s, x, params, P, sums);
  hipLaunchKernelGGL((aug_point_kernel<C, VP>), gp, block, 0, s, x, params, P, (const uint32_t*)sums, out, tmp, hist);
  hipLaunchKernelGGL((aug_sharp_kernel<C, VS>), gs, block, 0, s, (const uint8_t*)tmp, params, H, W, out, hist);
  hipLaunchKernelGGL((aug_equalize_kernel<C, VP>), gp, block, 0, s, out, params, P, (const uint32_t*)hist);
}

template <int C>
void launch_c(bool vec_plane, bool vec_row, hipStream_t s, const uint8_t* x, const float* params, int N, int H, int W, uint8_t* out,
              uint8_t* tmp, uint32_t* sums, uint32_t* hist) {
  if (vec_row) launch_all<C, 16, 16>(s, x, params, N, H, W, out, tmp, sums, hist);
  else if (vec_plane) launch_all<C, 16, 1>(s, x, params, N, H, W, out, tmp, sums, hist);
  else launch_all<C, 1, 1>(s, x, params, N, H, W, out, tmp, sums, hist);
}

inline size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool shape_ok(int N, int C, int H, int W) {
  return N > 0 && N <= 65535 && (C == 1 || C == 3) && H >= 3 && W >= 3 && (int64_t)H * W <= HD_AUG_MAX_PIXELS;
}

}  // namespace

extern "C" int64_t hd_augment_u8_ws_bytes(int N, int C, int H, int W) {
  if (!shape_ok(N, C, H, W)) {
    hd_set_error("hd_augment_u8_ws_bytes: need 1 <= N <= 65535, C in {1, 3}, H, W >= 3, H*W <= %d (got N=%d C=%d H=%d W=%d)",
                 HD_AUG_MAX_PIXELS, N, C, H, W);
    return HD_E_ARG;
  }
  return (int64_t)(round256((size_t)N * C * H * W) + round256(((size_t)N + (size_t)N * C * 256) * sizeof(uint32_t)));
}

extern "C" int hd_augment_u8(const uint8_t* x, const float* params, int N, int C, int H, int W, uint8_t* out, void* ws, void* stream) {
  HD_CHECK_ARG(x && params && out && ws, "hd_augment_u8: null pointer (x, params, out and ws are required)");
  HD_CHECK_ARG(shape_ok(N, C, H, W), "hd_augment_u8: need 1 <= N <= 65535, C in {1, 3}, H, W >= 3, H*W <= %d (got N=%d C=%d H=%d W=%d)",
               HD_AUG_MAX_PIXELS, N, C, H, W);
  HD_CHECK_ARG(hd_aligned16(ws), "hd_augment_u8: ws must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* tmp = (uint8_t*)ws;
  const size_t acc_words = (size_t)N + (size_t)N * C * 256;
  uint32_t* sums = (uint32_t*)((uint8_t*)ws + round256((size_t)N * C * H * W));
  uint32_t* hist = sums + N;
  if (hipMemsetAsync(sums, 0, acc_words * sizeof(uint32_t), s) != hipSuccess) {
    hd_set_error("hd_augment_u8: hipMemsetAsync failed");
    return HD_E_LAUNCH;
  }
  // 16 bytes per lane: the pointwise passes when every plane starts on a 16-byte boundary (H*W a multiple of 16: the three planes of a
  // pixel are then aligned alike), the sharpness pass when every row does (W a multiple of 16); one byte per lane otherwise
  const bool base16 = hd_aligned16(x) && hd_aligned16(out);
  const bool vec_plane = base16 && ((int64_t)H * W) % 16 == 0, vec_row = base16 && (W % 16) == 0;
  if (C == 3) launch_c<3>(vec_plane, vec_row, s, x, params, N, H, W, out, tmp, sums, hist);
  else launch_c<1>(vec_plane, vec_row, s, x, params, N, H, W, out, tmp, sums, hist);
  HD_CHECK_LAUNCH();
  return HD_OK;
}
