// Detector-input resize with separable tap tables (--detector-resize nearest | bilinear | bilinear_aa) and the per-channel
// normalisation of torchvision's GeneralizedRCNNTransform, fused with the NCHW fp32 -> NHWC (channels padded to 8) layout change:
//   y[n, ho, wo, c]  = sum_i sum_j wy[ho, i] * wx[wo, j] * (x[n, c, ys[ho] + i, xs[wo] + j] - mean[c]) * (1 / std[c])
//   dx[n, c, h, w]   = (gscale * (1 / std[c])) * sum over the outputs (ho, wo) that read (h, w) of wy * wx * dy[n, ho, wo, c]
// The weights come from host tables (hallucidet_amd/resample.py: float64 arithmetic, stored fp32): the kernels evaluate no source
// coordinate.  The forward table of an axis is (start[out], count[out], weight[out][T]); the gradient walks the SAME entries in
// transposed (CSR) form (rstart[in + 1], rout[nnz], rweight[nnz]), one writer per input pixel: no atomics, the same bits every run.
// Both sums run in fp32 instructions in a fixed order -- rows ascending, then columns ascending (no contraction: the library is built
// with -ffp-contract=off; the fused multiply-adds below are spelled out).  The gradient adds plain fp32 terms fl(fl(wy * wx) * g).
// The forward sum is carried as an unevaluated pair of floats (high + low part, error-free sums and products): an fp16 image of a
// normalised batch holds values far smaller than the terms that cancel to them (|x_norm| up to 2.6 with ImageNet statistics), and the
// stored value has to be an fp16 neighbour of the exact one down to the subnormals, which a plain fp32 sum (error 2^-24 of the largest
// term) and an fp32 table (the same again) cannot give.  So the forward table carries a low part, weight_lo = fp32(W - fp32(W)), the
// normalisation (x - mean) / std is evaluated as a pair, and what is stored is the high part of the sum: the exact result rounded once
// to fp32 (to within 2^-44 of the largest term), then to the storage type.
// With one tap of weight 1, mean 0 and std 1 both kernels reproduce hd_nchw_to_nhwc_resize / _bwd bit for bit.
// Whatever a table holds, no address leaves x or dy: starts, counts and transposed indices are clamped to the extents the caller
// passed before they are used (the tables themselves are checked on the host: hd_resample_taps_check).
#include "hd_common.h"

namespace {

constexpr int TB = 256;
constexpr int MAX_TAPS = 32;
constexpr int MAX_C = 8;

struct ChanStats {           // by value in the kernel arguments: mean, std and fl(1 / std) of the (at most 8) real channels
  float mean[MAX_C];
  float std_[MAX_C];
  float inv_std[MAX_C];
};

// a value carried as h + l, |l| <= ulp(h) / 2
struct f32p {
  float h, l;
};
// s + e == a + b exactly
__device__ __forceinline__ f32p two_sum(float a, float b) {
  const float s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
// the same for |a| >= |b| (or a == 0)
__device__ __forceinline__ f32p fast_two_sum(float a, float b) {
  const float s = a + b;
  return {s, b - (s - a)};
}
// (ah + al) * (bh + bl), relative error of the order 2^-46
__device__ __forceinline__ f32p pair_mul(float ah, float al, float bh, float bl) {
  const float p = ah * bh;
  float e = __builtin_fmaf(ah, bh, -p);
  e = e + (ah * bl + al * bh);
  return e != 0.f ? fast_two_sum(p, e) : f32p{p, 0.f};
}

inline int grid_for(int64_t work, int per_block = TB, int cap = 256 * 16) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One thread per output pixel; CR = compile-time bound of the real channel count (3: images, 8: anything the layout allows).
template <int CR>
__global__ __launch_bounds__(TB) void image_resample_kernel(const float* __restrict__ x, int64_t nstride, int64_t cstride,
                                                            f16* __restrict__ y, int N, int Cr, int H, int W, int Ho, int Wo,
                                                            const int* __restrict__ ystart, const int* __restrict__ ycount,
                                                            const float* __restrict__ yweight, int Ty,
                                                            const int* __restrict__ xstart, const int* __restrict__ xcount,
                                                            const float* __restrict__ xweight, int Tx,
                                                            const float* __restrict__ yweight_lo, const float* __restrict__ xweight_lo,
                                                            ChanStats st) {
  const int64_t total = (int64_t)N * Ho * Wo;
  for (int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x; p < total; p += (int64_t)gridDim.x * TB) {
    const int wo = (int)(p % Wo);
    const int ho = (int)((p / Wo) % Ho);
    const int n = (int)(p / ((int64_t)Wo * Ho));
    const int ys = clampi(ystart[ho], 0, H - 1), yc = clampi(ycount[ho], 0, Ty);
    const int xs = clampi(xstart[wo], 0, W - 1), xc = clampi(xcount[wo], 0, Tx);
    const float* wyp = yweight + (int64_t)ho * Ty;
    const float* wxp = xweight + (int64_t)wo * Tx;
    const float* xn = x + (int64_t)n * nstride;
    const float* wylp = yweight_lo ? yweight_lo + (int64_t)ho * Ty : nullptr;      // a table without low parts: they are zero
    const float* wxlp = xweight_lo ? xweight_lo + (int64_t)wo * Tx : nullptr;
    float acc[CR], accl[CR];
#pragma unroll
    for (int c = 0; c < CR; ++c) {
      acc[c] = -0.f;                                     // -0 + v == v for every v, signed zeros included
      accl[c] = 0.f;
    }
    for (int i = 0; i < yc; ++i) {
      const int h = min(ys + i, H - 1);
      const float wy = wyp[i], wyl = wylp ? wylp[i] : 0.f;
      const float* row = xn + (int64_t)h * W;
      for (int j = 0; j < xc; ++j) {
        const int w = min(xs + j, W - 1);
        const f32p wt = pair_mul(wy, wyl, wxp[j], wxlp ? wxlp[j] : 0.f);
#pragma unroll
        for (int c = 0; c < CR; ++c) {
          if (c < Cr) {
            // v = (x - mean) / std as a pair: the difference exactly, the quotient by one correction step on fl(d * fl(1 / std))
            const f32p d = two_sum(row[(int64_t)c * cstride + w], -st.mean[c]);
            const float qh = d.h * st.inv_std[c];
            const float ql = (__builtin_fmaf(-qh, st.std_[c], d.h) + d.l) * st.inv_std[c];
            const f32p v = ql != 0.f ? fast_two_sum(qh, ql) : f32p{qh, 0.f};
            const f32p t = pair_mul(wt.h, wt.l, v.h, v.l);
            const f32p s = two_sum(acc[c], t.h);
            const float e = s.l + (accl[c] + t.l);
            if (e != 0.f) {
              const f32p r = fast_two_sum(s.h, e);
              acc[c] = r.h;
              accl[c] = r.l;
            } else {
              acc[c] = s.h;
              accl[c] = 0.f;
            }
          }
        }
      }
    }
    f16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (f16)0.f;
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < Cr) o[c] = (f16)acc[c];                    // the high part: the sum rounded to fp32
    *reinterpret_cast<f16x8*>(y + p * 8) = o;            // one 16-byte store per pixel (two in the fp32-storage build)
  }
}

// One thread per input position (n, h, w): every dx element has one writer.
template <int CR>
__global__ __launch_bounds__(TB) void image_resample_bwd_kernel(const f16* __restrict__ dy, float* __restrict__ dx, int N, int Cr, int H, int W,
                                                                int Ho, int Wo, const int* __restrict__ yrstart, const int* __restrict__ yrout,
                                                                const float* __restrict__ yrweight, int ynnz,
                                                                const int* __restrict__ xrstart, const int* __restrict__ xrout,
                                                                const float* __restrict__ xrweight, int xnnz, ChanStats st, float gscale) {
  const int64_t total = (int64_t)N * H * W;
  for (int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x; p < total; p += (int64_t)gridDim.x * TB) {
    const int w = (int)(p % W);
    const int h = (int)((p / W) % H);
    const int n = (int)(p / ((int64_t)W * H));
    const int yb = clampi(yrstart[h], 0, ynnz), ye = clampi(yrstart[h + 1], yb, ynnz);
    const int xb = clampi(xrstart[w], 0, xnnz), xe = clampi(xrstart[w + 1], xb, xnnz);
    float acc[CR];
#pragma unroll
    for (int c = 0; c < CR; ++c) acc[c] = 0.f;
    for (int a = yb; a < ye; ++a) {
      const int ho = clampi(yrout[a], 0, Ho - 1);
      const float wy = yrweight[a];
      const f16* grow = dy + ((int64_t)n * Ho + ho) * Wo * 8;
      for (int b = xb; b < xe; ++b) {
        const int wo = clampi(xrout[b], 0, Wo - 1);
        const float wt = wy * xrweight[b];
        const f16x8 g = *reinterpret_cast<const f16x8*>(grow + (int64_t)wo * 8);
#pragma unroll
        for (int c = 0; c < CR; ++c) acc[c] += wt * (float)g[c];
      }
    }
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < Cr) dx[(((int64_t)n * Cr + c) * H + h) * W + w] = acc[c] * (gscale * st.inv_std[c]);
  }
}

// mean may be NULL (0); std may be NULL (1).  1 / std is rounded once, here.
inline bool fill_stats(ChanStats& st, const float* mean, const float* std_, int Cr) {
  for (int c = 0; c < MAX_C; ++c) {
    st.mean[c] = 0.f;
    st.std_[c] = 1.f;
    st.inv_std[c] = 1.f;
  }
  for (int c = 0; c < Cr; ++c) {
    if (mean) st.mean[c] = mean[c];
    if (std_) {
      if (!(std_[c] > 0.f) || !(std_[c] < 3.0e38f)) return false;
      st.std_[c] = std_[c];
      st.inv_std[c] = 1.f / std_[c];
    }
    if (!(st.mean[c] == st.mean[c]) || !(st.mean[c] > -3.0e38f && st.mean[c] < 3.0e38f)) return false;
  }
  return true;
}

}  // namespace

extern "C" int HD_API(hd_image_resample)(const float* x, int64_t nstride, int64_t cstride, void* y, int N, int Cr, int H, int W, int Ho, int Wo,
                                         int Cp, const int* ystart, const int* ycount, const float* yweight, int Ty, const int* xstart,
                                         const int* xcount, const float* xweight, int Tx, const float* mean, const float* std_,
                                         const float* yweight_lo, const float* xweight_lo, void* stream) {
  HD_CHECK_ARG(x && y, "hd_image_resample: null pointer (x and y are required)");
  HD_CHECK_ARG(ystart && ycount && yweight && xstart && xcount && xweight, "hd_image_resample: null tap table");
  HD_CHECK_ARG(N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "hd_image_resample: bad shape N=%d H=%d W=%d Ho=%d Wo=%d", N, H, W, Ho, Wo);
  HD_CHECK_ARG(Cp == 8 && Cr >= 1 && Cr <= MAX_C, "hd_image_resample: Cp must be 8 and 1 <= Cr <= 8 (got Cp=%d Cr=%d)", Cp, Cr);
  HD_CHECK_ARG(Ty >= 1 && Ty <= MAX_TAPS && Tx >= 1 && Tx <= MAX_TAPS, "hd_image_resample: 1 .. %d taps per axis (got Ty=%d Tx=%d)", MAX_TAPS, Ty, Tx);
  HD_CHECK_ARG(cstride == 0 || cstride >= (int64_t)H * W, "hd_image_resample: cstride must be 0 or >= H*W (got %lld)", (long long)cstride);
  HD_CHECK_ARG(nstride >= 0 && (N == 1 || nstride >= (int64_t)H * W), "hd_image_resample: nstride must be >= H*W (got %lld)", (long long)nstride);
  HD_CHECK_ARG((reinterpret_cast<uintptr_t>(y) & 15) == 0, "hd_image_resample: y must be 16-byte aligned");
  HD_CHECK_ARG((yweight_lo == nullptr) == (xweight_lo == nullptr), "hd_image_resample: weight_lo tables go together (both or neither)");
  ChanStats st;
  HD_CHECK_ARG(fill_stats(st, mean, std_, Cr), "hd_image_resample: mean must be finite and std finite and > 0");
  const int grid = grid_for((int64_t)N * Ho * Wo);
  hipStream_t s = (hipStream_t)stream;
  if (Cr <= 3)
    hipLaunchKernelGGL((image_resample_kernel<3>), dim3(grid), dim3(TB), 0, s, x, nstride, cstride, (f16*)y, N, Cr, H, W, Ho, Wo, ystart, ycount,
                       yweight, Ty, xstart, xcount, xweight, Tx, yweight_lo, xweight_lo, st);
  else
    hipLaunchKernelGGL((image_resample_kernel<8>), dim3(grid), dim3(TB), 0, s, x, nstride, cstride, (f16*)y, N, Cr, H, W, Ho, Wo, ystart, ycount,
                       yweight, Ty, xstart, xcount, xweight, Tx, yweight_lo, xweight_lo, st);
  HD_CHECK_LAUNCH();
  return HD_OK;
}

extern "C" int HD_API(hd_image_resample_bwd)(const void* dy, float* dx, int N, int Cr, int H, int W, int Ho, int Wo, int Cp, const int* yrstart,
                                             const int* yrout, const float* yrweight, int ynnz, const int* xrstart, const int* xrout,
                                             const float* xrweight, int xnnz, const float* std_, float gscale, void* stream) {
  HD_CHECK_ARG(dy && dx, "hd_image_resample_bwd: null pointer (dy and dx are required)");
  HD_CHECK_ARG(yrstart && yrout && yrweight && xrstart && xrout && xrweight, "hd_image_resample_bwd: null tap table");
  HD_CHECK_ARG(N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "hd_image_resample_bwd: bad shape N=%d H=%d W=%d Ho=%d Wo=%d", N, H, W, Ho, Wo);
  HD_CHECK_ARG(Cp == 8 && Cr >= 1 && Cr <= MAX_C, "hd_image_resample_bwd: Cp must be 8 and 1 <= Cr <= 8 (got Cp=%d Cr=%d)", Cp, Cr);
  HD_CHECK_ARG(ynnz >= 1 && xnnz >= 1 && (int64_t)ynnz <= (int64_t)Ho * MAX_TAPS && (int64_t)xnnz <= (int64_t)Wo * MAX_TAPS,
               "hd_image_resample_bwd: 1 .. out * %d table entries per axis (got ynnz=%d xnnz=%d)", MAX_TAPS, ynnz, xnnz);
  HD_CHECK_ARG((reinterpret_cast<uintptr_t>(dy) & 15) == 0, "hd_image_resample_bwd: dy must be 16-byte aligned");
  ChanStats st;
  HD_CHECK_ARG(fill_stats(st, nullptr, std_, Cr), "hd_image_resample_bwd: std must be finite and > 0");
  const int grid = grid_for((int64_t)N * H * W);
  hipStream_t s = (hipStream_t)stream;
  if (Cr <= 3)
    hipLaunchKernelGGL((image_resample_bwd_kernel<3>), dim3(grid), dim3(TB), 0, s, (const f16*)dy, dx, N, Cr, H, W, Ho, Wo, yrstart, yrout, yrweight,
                       ynnz, xrstart, xrout, xrweight, xnnz, st, gscale);
  else
    hipLaunchKernelGGL((image_resample_bwd_kernel<8>), dim3(grid), dim3(TB), 0, s, (const f16*)dy, dx, N, Cr, H, W, Ho, Wo, yrstart, yrout, yrweight,
                       ynnz, xrstart, xrout, xrweight, xnnz, st, gscale);
  HD_CHECK_LAUNCH();
  return HD_OK;
}

#ifndef HD_STORE_F32
// Host-side check of one axis' tables (HOST pointers), to be called before they are uploaded: every forward tap lies inside the input,
// every transposed entry names an output, rows are sorted by output index, and the transposed form lists exactly the forward form's entries.
extern "C" int hd_resample_taps_check(const int* start, const int* count, const float* weight, int in_size, int out_size, int T, const int* rstart,
                                      const int* rout, const float* rweight, int nnz, const float* weight_lo) {
  HD_CHECK_ARG(start && count && weight && rstart && rout && rweight, "hd_resample_taps_check: null pointer");
  HD_CHECK_ARG(in_size >= 1 && out_size >= 1, "hd_resample_taps_check: sizes must be >= 1 (got in=%d out=%d)", in_size, out_size);
  HD_CHECK_ARG(T >= 1 && T <= MAX_TAPS, "hd_resample_taps_check: 1 .. %d taps (got %d)", MAX_TAPS, T);
  int64_t entries = 0;
  for (int o = 0; o < out_size; ++o) {
    HD_CHECK_ARG(count[o] >= 1 && count[o] <= T, "hd_resample_taps_check: count[%d] = %d outside 1 .. %d", o, count[o], T);
    HD_CHECK_ARG(start[o] >= 0 && (int64_t)start[o] + count[o] <= in_size, "hd_resample_taps_check: taps of output %d (%d .. %d) leave the input (%d)", o,
                 start[o], start[o] + count[o] - 1, in_size);
    for (int i = 0; i < T; ++i) {
      const float wv = weight[(int64_t)o * T + i];
      HD_CHECK_ARG(wv == wv && wv > -3.0e38f && wv < 3.0e38f, "hd_resample_taps_check: weight[%d][%d] is not finite", o, i);
      HD_CHECK_ARG(i < count[o] || wv == 0.f, "hd_resample_taps_check: weight[%d][%d] past the count is not zero", o, i);
      if (weight_lo) {          // the low part refines the weight: at most half a unit in its last place
        const float lv = weight_lo[(int64_t)o * T + i];
        HD_CHECK_ARG(lv == lv && (lv < 0.f ? -lv : lv) <= 5.9604645e-8f * (wv < 0.f ? -wv : wv),
                     "hd_resample_taps_check: weight_lo[%d][%d] is no low part of the weight", o, i);
      }
    }
    entries += count[o];
  }
  HD_CHECK_ARG(nnz == entries, "hd_resample_taps_check: the transposed form has %d entries, the forward form %lld", nnz, (long long)entries);
  HD_CHECK_ARG(rstart[0] == 0 && rstart[in_size] == nnz, "hd_resample_taps_check: rstart must run from 0 to nnz");
  for (int r = 0; r < in_size; ++r) {
    HD_CHECK_ARG(rstart[r] <= rstart[r + 1], "hd_resample_taps_check: rstart decreases at %d", r);
    HD_CHECK_ARG(rstart[r + 1] <= nnz, "hd_resample_taps_check: rstart[%d] beyond nnz", r + 1);
    for (int a = rstart[r]; a < rstart[r + 1]; ++a) {
      const int o = rout[a];
      HD_CHECK_ARG(o >= 0 && o < out_size, "hd_resample_taps_check: rout[%d] = %d outside the output (%d)", a, o, out_size);
      HD_CHECK_ARG(a == rstart[r] || rout[a - 1] < o, "hd_resample_taps_check: row %d is not sorted by output index", r);
      const int i = r - start[o];
      HD_CHECK_ARG(i >= 0 && i < count[o], "hd_resample_taps_check: entry %d (input %d, output %d) is no forward tap", a, r, o);
      const float fw = weight[(int64_t)o * T + i];
      HD_CHECK_ARG(fw == rweight[a], "hd_resample_taps_check: entry %d differs from the forward weight", a);
    }
  }
  return HD_OK;
}
#endif
