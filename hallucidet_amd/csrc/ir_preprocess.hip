// Image-space IR pre-processing baselines of the reference (src/models/cnnBasedThermalInfraredDA.py, after Herrmann et al.: invert,
// histogram stretching, histogram equalization, 3 x 3 Gaussian blur and their chains) on the fp32 batch in HBM.
// Images are planar fp32 [N][C][H][W], C = 3 or 1; every operation works per image and per channel.  A call takes a HOST list of up
// to four stages `op | channel_mask << 8`; a channel outside a stage's mask passes through that stage.  The list is turned into
// passes on the host, so the launch sequence depends on the list alone (not on the data, not on N):
//   invert     never a pass of its own: the inverts in front of a stretch / equalize / blur stage are applied where that stage READS
//              its input, the ones behind the last such stage where it WRITES its output; a list of inverts alone is one pointwise pass
//   stretch    exact order statistics by radix select over the monotone integer image of the float bits, 8 bits per level:
//              4 x (histogram pass, one-block-per-plane resolve), then one pointwise pass  y = clamp((x - q_min) / (q_max - q_min),
//              q_min, q_max)  (the reference clamps to the quantiles; a constant plane is 0/0 = NaN and stays NaN)
//   equalize   u = trunc(x * 255) (one fp32 product, then the cast), 256-bin histogram pass, then one pointwise pass whose blocks
//              each build torchvision's look-up table from the histogram (block scan) and write float(lut[u]) / 255
//   blur       one stencil pass over the previous pass's materialised output, reflect indexing (no edge repeat)
// Pass k reads the previous pass's output; outputs alternate between `out` and one workspace buffer so that the last lands in `out`.
// The accumulators are cleared by one launch in front of the first pass.  Histograms are 32-bit integer counts (registers -> LDS ->
// one global atomic per block and bin): the result does not depend on the order of arrival.  Every fp32 step below is one IEEE
// operation: no contraction, true divisions.
#include "hd_block.h"
#pragma clang fp contract(off)

namespace {

constexpr int TB = 256;            // threads per block
constexpr int MAXBX_HIST = 32;     // most blocks per plane of a histogram pass: long per-thread runs, few LDS atomics
constexpr int MAXBX = 128;         // most blocks per plane of a pointwise / stencil pass
constexpr int OP_COPY = -1;        // the pointwise pass of a list without stretch / equalize / blur

// accumulator words of one (stage, plane)
constexpr int A_HIST0 = 0;                 // level-0 histogram of the radix select (one for the four targets) / equalize histogram
constexpr int A_HISTL = 256;               // levels 1..3: [level - 1][target][256]
constexpr int A_PREFIX = 256 + 3 * 4 * 256;  // [4] key prefix of each target after the resolved levels
constexpr int A_REM = A_PREFIX + 4;        // [4] rank of each target among the keys that share its prefix
constexpr int A_Q = A_REM + 4;             // [2] q_min, q_max (float bits)
constexpr int A_WORDS = A_Q + 8;           // 3344, a multiple of 4

// the two quantile levels of the reference (beta = 0.003): q and 1 - q as torch.quantile sees them, doubles rounded to fp32
constexpr float Q_LO = (float)0.003;
constexpr float Q_HI = (float)(1.0 - 0.003);

// torchvision gaussian_blur, kernel 3 x 3, sigma = 0.8: 1-D taps exp(-0.5 (t / sigma)^2) / sum in fp32, 2-D = outer product in fp32
constexpr float G_A = 0x1.e975d4p-3f, G_B = 0x1.0b4518p-1f;
constexpr float W_AA = G_A * G_A, W_AB = G_A * G_B, W_BB = G_B * G_B;

__device__ __forceinline__ float invert_n(float v, int n) {
  for (int i = 0; i < n; ++i) v = 1.0f - v;
  return v;
}

// (x * 255) truncated to uint8; values outside [0, 1] (unspecified input) are held inside the table
__device__ __forceinline__ int quantise(float v) {
  const float s = v * 255.0f;
  const int u = (int)s;
  return u < 0 ? 0 : (u > 255 ? 255 : u);
}

// run-length front of an LDS histogram: a thread's consecutive hits of one bin cost one atomic (8-bit images and the exponent byte
// of [0, 1] data put most pixels into a handful of bins)
struct Run {
  int bin = -1;
  uint32_t n = 0u;
  __device__ __forceinline__ void add(uint32_t* sh, int b) {
    if (b == bin) {
      ++n;
    } else {
      if (n) atomicAdd(&sh[bin], n);
      bin = b;
      n = 1u;
    }
  }
  __device__ __forceinline__ void flush(uint32_t* sh) {
    if (n) atomicAdd(&sh[bin], n);
  }
};

// ---- clear the accumulators (a launch of the list rather than a memset, so that a captured call replays it like every other pass)
__global__ __launch_bounds__(TB) void irp_clear_kernel(u32x4* __restrict__ acc, size_t n4) {
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < n4; i += (size_t)gridDim.x * TB) acc[i] = z;
}

// ---- histogram pass.  level 0..3: radix-select level (bits 31-8*level .. 24-8*level of the key, for the keys under each target's
// prefix); level < 0: the equalize histogram.  grid = (blocks, planes); planes outside the mask leave at once.
template <int V>
__global__ __launch_bounds__(TB) void irp_hist_kernel(const float* __restrict__ src, uint32_t* __restrict__ acc, int C, int mask, int pre,
                                                      int level, int P) {
  const int plane = blockIdx.y, c = plane % C;
  if (!((mask >> c) & 1)) return;
  __shared__ uint32_t sh[4 * 256];
  const int nbins = level > 0 ? 4 * 256 : 256;
  for (int i = threadIdx.x; i < nbins; i += TB) sh[i] = 0u;
  __syncthreads();
  uint32_t* a = acc + (size_t)plane * A_WORDS;
  const int npre = (pre >> (4 * c)) & 15;
  const float* pl = src + (size_t)plane * P;
  const int groups = P / V;
  if (level <= 0) {
    Run run;
    for (int g = blockIdx.x * TB + threadIdx.x; g < groups; g += gridDim.x * TB) {
      float v[V];
      hd_ldv<V>(pl + (size_t)g * V, v);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float t = invert_n(v[k], npre);
        run.add(sh, level < 0 ? quantise(t) : (int)(hd_float_key(t) >> 24));
      }
    }
    run.flush(sh);
  } else {
    const uint32_t p0 = a[A_PREFIX], p1 = a[A_PREFIX + 1], p2 = a[A_PREFIX + 2], p3 = a[A_PREFIX + 3];
    const int shift = 24 - 8 * level;
    Run r0, r1, r2, r3;
    for (int g = blockIdx.x * TB + threadIdx.x; g < groups; g += gridDim.x * TB) {
      float v[V];
      hd_ldv<V>(pl + (size_t)g * V, v);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const uint32_t key = hd_float_key(invert_n(v[k], npre));
        const uint32_t pfx = key >> (shift + 8);
        const int d = (int)((key >> shift) & 255u);
        if (pfx == p0) r0.add(sh, d);
        if (pfx == p1) r1.add(sh, 256 + d);
        if (pfx == p2) r2.add(sh, 512 + d);
        if (pfx == p3) r3.add(sh, 768 + d);
      }
    }
    r0.flush(sh); r1.flush(sh); r2.flush(sh); r3.flush(sh);
  }
  __syncthreads();
  uint32_t* gh = level > 0 ? a + A_HISTL + (level - 1) * 4 * 256 : a + A_HIST0;
  for (int i = threadIdx.x; i < nbins; i += TB) {
    const uint32_t v = sh[i];
    if (v) atomicAdd(gh + i, v);
  }
}

// ---- resolve one level of the radix select: one block per plane, wave t = target t (lo and hi neighbour of the lower quantile, lo
// and hi neighbour of the upper one).  rank = fp32(q) * fp32(n - 1) in fp32, lo = floor(rank), hi = min(lo + 1, n - 1).  After level 3
// the four prefixes are the keys of the exact input elements at those ranks; thread 0 interpolates (ATen's lerp, one rounding per
// operation) and writes q_min, q_max.
__global__ __launch_bounds__(TB) void irp_resolve_kernel(uint32_t* __restrict__ acc, int C, int mask, int level, int P,
                                                         float* __restrict__ q_out) {
  static_assert(TB == 256, "four waves, one per target");
  const int plane = blockIdx.x, c = plane % C;
  if (!((mask >> c) & 1)) return;
  __shared__ float vals[4];
  uint32_t* a = acc + (size_t)plane * A_WORDS;
  const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float nm1 = (float)(P - 1);
  const float rank = (t < 2 ? Q_LO : Q_HI) * nm1;
  const float lo_f = floorf(rank);
  uint32_t prefix = 0u, rem;
  if (level == 0) {
    const int lo = (int)lo_f;
    const int hi = lo + 1 < P ? lo + 1 : P - 1;
    rem = (uint32_t)((t & 1) ? hi : lo);
  } else {
    prefix = a[A_PREFIX + t];
    rem = a[A_REM + t];
  }
  const uint32_t* h = level == 0 ? a + A_HIST0 : a + A_HISTL + ((level - 1) * 4 + t) * 256;
  const uint32_t b0 = h[4 * lane], b1 = h[4 * lane + 1], b2 = h[4 * lane + 2], b3 = h[4 * lane + 3];
  const uint32_t s = b0 + b1 + b2 + b3;
  const uint32_t incl = hd_wave_scan(s, lane);
  uint32_t e = incl - s;
  if (rem >= e && rem < incl) {          // one lane of the wave
    int d = 0;
    if (rem >= e + b0) {
      e += b0; d = 1;
      if (rem >= e + b1) {
        e += b1; d = 2;
        if (rem >= e + b2) {
          e += b2; d = 3;
        }
      }
    }
    const uint32_t np = (prefix << 8) | (uint32_t)(4 * lane + d);
    a[A_PREFIX + t] = np;
    a[A_REM + t] = rem - e;
    if (level == 3) vals[t] = hd_key_float(np);
  }
  if (level != 3) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    float q[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float r = (j == 0 ? Q_LO : Q_HI) * nm1;
      const float w = r - floorf(r);
      const float lo = vals[2 * j], hi = vals[2 * j + 1];
      const float diff = hi - lo;
      if (w < 0.5f) {
        const float m = w * diff;
        q[j] = lo + m;
      } else {
        const float omw = 1.0f - w;
        const float m = diff * omw;
        q[j] = hi - m;
      }
    }
    a[A_Q] = __float_as_uint(q[0]);
    a[A_Q + 1] = __float_as_uint(q[1]);
    if (q_out) {
      q_out[(size_t)plane * 2] = q[0];
      q_out[(size_t)plane * 2 + 1] = q[1];
    }
  }
}

// ---- pointwise pass: inverts of the read side, the operation on the planes of its mask, inverts of the write side
template <int V>
__global__ __launch_bounds__(TB) void irp_point_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                       const uint32_t* __restrict__ acc, int C, int op, int mask, int pre, int post, int P) {
  static_assert(TB == 256, "one thread per histogram bin");
  const int plane = blockIdx.y, c = plane % C;
  const bool active = op != OP_COPY && ((mask >> c) & 1);
  const bool stretch = active && op == HD_IRP_STRETCH, equalize = active && op == HD_IRP_EQUALIZE;
  const int npre = (pre >> (4 * c)) & 15, npost = (post >> (4 * c)) & 15;
  __shared__ float lut[256];
  __shared__ uint32_t wsum[4];
  __shared__ int wlast[4];
  float q_min = 0.f, q_max = 0.f, den = 1.f;
  if (stretch) {
    const uint32_t* a = acc + (size_t)plane * A_WORDS;
    q_min = __uint_as_float(a[A_Q]);
    q_max = __uint_as_float(a[A_Q + 1]);
    den = q_max - q_min;
  }
  if (equalize) {
    // torchvision equalize: step = (pixels outside the last non-empty bin) // 255; step == 0: identity table; else
    // lut[i] = min((sum of the bins below i + step // 2) // step, 255)
    const int i = threadIdx.x, w = i >> 6, lane = i & 63;
    const uint32_t h = acc[(size_t)plane * A_WORDS + A_HIST0 + i];
    const uint32_t incl = hd_wave_scan(h, lane);
    int last = hd_wave_reduce(h ? i : -1, HdMax());
    if (lane == 63) wsum[w] = incl;
    if (lane == 0) wlast[w] = last;
    __syncthreads();
    uint32_t below = incl - h;
    for (int j = 0; j < w; ++j) below += wsum[j];
    last = max(max(wlast[0], wlast[1]), max(wlast[2], wlast[3]));
    const uint32_t h_last = last >= 0 ? acc[(size_t)plane * A_WORDS + A_HIST0 + last] : 0u;
    const uint32_t step = ((uint32_t)P - h_last) / 255u;
    int v = i;
    if (step != 0u) {
      const uint32_t q = (below + step / 2u) / step;
      v = q > 255u ? 255 : (int)q;
    }
    lut[i] = (float)v / 255.0f;
    __syncthreads();
  }
  const float* pi = src + (size_t)plane * P;
  float* po = dst + (size_t)plane * P;
  const int groups = P / V;
  for (int g = blockIdx.x * TB + threadIdx.x; g < groups; g += gridDim.x * TB) {
    float v[V];
    hd_ldv<V>(pi + (size_t)g * V, v);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float t = invert_n(v[k], npre);
      if (stretch) {
        const float num = t - q_min;
        const float y = num / den;
        t = y < q_min ? q_min : (y > q_max ? q_max : y);      // NaN fails both comparisons and stays
      } else if (equalize) {
        t = lut[quantise(t)];
      }
      v[k] = invert_n(t, npost);
    }
    hd_stv<V>(po + (size_t)g * V, v);
  }
}

// ---- 3 x 3 Gaussian, reflect indexing (-1 -> 1, H -> H - 2).  The nine fp32 products weight * value are formed one by one and summed
// in row-major tap order: ((((((((w00 v00 + w01 v01) + w02 v02) + w10 v10) + w11 v11) + w12 v12) + w20 v20) + w21 v21) + w22 v22).
// V == 4 only with W % 4 == 0: a group lies in one row.
template <int V>
__global__ __launch_bounds__(TB) void irp_blur_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int mask, int pre, int post,
                                                      int H, int W) {
  const int plane = blockIdx.y, c = plane % C;
  const bool active = (mask >> c) & 1;
  const int npre = (pre >> (4 * c)) & 15, npost = (post >> (4 * c)) & 15;
  const int P = H * W;
  const float* pl = src + (size_t)plane * P;
  float* po = dst + (size_t)plane * P;
  const int groups = P / V;
  for (int g = blockIdx.x * TB + threadIdx.x; g < groups; g += gridDim.x * TB) {
    const int p0 = g * V;
    float mid[V], res[V];
    hd_ldv<V>(pl + p0, mid);
#pragma unroll
    for (int k = 0; k < V; ++k) mid[k] = invert_n(mid[k], npre);
    if (active) {
      const int y = p0 / W, x0 = p0 - y * W;
      const int ym = y > 0 ? y - 1 : 1, yp = y < H - 1 ? y + 1 : H - 2;
      const int xl = x0 > 0 ? x0 - 1 : 1, xr = x0 + V < W ? x0 + V : W - 2;
      const float* ru = pl + (size_t)ym * W;
      const float* rm = pl + (size_t)y * W;
      const float* rd = pl + (size_t)yp * W;
      float up[V], dn[V];
      hd_ldv<V>(ru + x0, up);
      hd_ldv<V>(rd + x0, dn);
      float l3[3] = {ru[xl], rm[xl], rd[xl]}, r3[3] = {ru[xr], rm[xr], rd[xr]};
#pragma unroll
      for (int k = 0; k < V; ++k) {
        up[k] = invert_n(up[k], npre);
        dn[k] = invert_n(dn[k], npre);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        l3[j] = invert_n(l3[j], npre);
        r3[j] = invert_n(r3[j], npre);
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float a0 = k > 0 ? up[k > 0 ? k - 1 : 0] : l3[0], a2 = k < V - 1 ? up[k < V - 1 ? k + 1 : 0] : r3[0];
        const float b0 = k > 0 ? mid[k > 0 ? k - 1 : 0] : l3[1], b2 = k < V - 1 ? mid[k < V - 1 ? k + 1 : 0] : r3[1];
        const float c0 = k > 0 ? dn[k > 0 ? k - 1 : 0] : l3[2], c2 = k < V - 1 ? dn[k < V - 1 ? k + 1 : 0] : r3[2];
        float s = W_AA * a0;
        float t;
        t = W_AB * up[k];  s = s + t;
        t = W_AA * a2;     s = s + t;
        t = W_AB * b0;     s = s + t;
        t = W_BB * mid[k]; s = s + t;
        t = W_AB * b2;     s = s + t;
        t = W_AA * c0;     s = s + t;
        t = W_AB * dn[k];  s = s + t;
        t = W_AA * c2;     s = s + t;
        res[k] = invert_n(s, npost);
      }
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) res[k] = invert_n(mid[k], npost);
    }
    hd_stv<V>(po + p0, res);
  }
}

struct Pass {
  int op, mask, pre, post;
};

inline size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool shape_ok(int N, int C, int H, int W, int n_stage) {
  return N > 0 && (C == 1 || C == 3) && (int64_t)N * C <= 65535 && H >= 2 && W >= 2 && (int64_t)H * W <= HD_IRP_MAX_PIXELS && n_stage >= 1 &&
         n_stage <= HD_IRP_MAX_STAGES;
}
inline size_t tmp_bytes(int N, int C, int H, int W, int n_stage) {
  return n_stage >= 2 ? round256((size_t)N * C * H * W * sizeof(float)) : 0;
}
inline dim3 grid_for(int P, int V, int planes, int maxbx) {
  const int gx = hd_cdiv(P / V, TB);
  return dim3(gx > maxbx ? maxbx : gx, planes);
}

#define SHAPE_MSG "need N >= 1, C in {1, 3}, N*C <= 65535, H, W >= 2, H*W <= %d, 1 <= n_stage <= %d (got N=%d C=%d H=%d W=%d n_stage=%d)"

}  // namespace

extern "C" int64_t hd_ir_preprocess_ws_bytes(int N, int C, int H, int W, int n_stage) {
  if (!shape_ok(N, C, H, W, n_stage)) {
    hd_set_error("hd_ir_preprocess_ws_bytes: " SHAPE_MSG, HD_IRP_MAX_PIXELS, HD_IRP_MAX_STAGES, N, C, H, W, n_stage);
    return HD_E_ARG;
  }
  return (int64_t)(tmp_bytes(N, C, H, W, n_stage) + round256((size_t)n_stage * N * C * A_WORDS * sizeof(uint32_t)));
}

extern "C" int hd_ir_preprocess(const float* x, int N, int C, int H, int W, const int* stages, int n_stage, float* out, float* q_out,
                                void* ws, void* stream) {
  HD_CHECK_ARG(x && stages && out && ws, "hd_ir_preprocess: null pointer (x, stages, out and ws are required)");
  HD_CHECK_ARG(shape_ok(N, C, H, W, n_stage), "hd_ir_preprocess: " SHAPE_MSG, HD_IRP_MAX_PIXELS, HD_IRP_MAX_STAGES, N, C, H, W, n_stage);
  HD_CHECK_ARG(x != out, "hd_ir_preprocess: out must not be x");
  HD_CHECK_ARG(hd_aligned16(ws), "hd_ir_preprocess: ws must be 16-byte aligned");
  // stage list -> passes: inverts wait (a count per channel, 4 bits each) for the next stage that reads or, at the end, the last that wrote
  Pass passes[HD_IRP_MAX_STAGES];
  int n_pass = 0, pending = 0;
  for (int i = 0; i < n_stage; ++i) {
    const int op = stages[i] & 255, mask = (stages[i] >> 8) & ((1 << C) - 1);
    HD_CHECK_ARG(stages[i] >= 0 && (stages[i] >> 11) == 0 && op <= HD_IRP_BLUR, "hd_ir_preprocess: stage %d = 0x%x is not op | channel_mask << 8 "
                 "with op in 0..3 and a 3-bit mask", i, stages[i]);
    HD_CHECK_ARG(mask != 0, "hd_ir_preprocess: stage %d names no channel of a %d-channel batch (mask 0x%x)", i, C, stages[i] >> 8);
    if (op == HD_IRP_INVERT) {
      for (int c = 0; c < C; ++c)
        if ((mask >> c) & 1) pending += 1 << (4 * c);
    } else {
      passes[n_pass++] = Pass{op, mask, pending, 0};
      pending = 0;
    }
  }
  if (n_pass == 0) passes[n_pass++] = Pass{OP_COPY, 0, pending, 0};
  else passes[n_pass - 1].post = pending;

  hipStream_t s = (hipStream_t)stream;
  const int P = H * W, planes = N * C;
  float* tmp = (float*)ws;
  uint32_t* acc = (uint32_t*)((uint8_t*)ws + tmp_bytes(N, C, H, W, n_stage));
  const size_t acc_stage = (size_t)planes * A_WORDS;
  if (passes[0].op != OP_COPY) {
    const size_t n4 = (size_t)n_pass * acc_stage / 4;          // A_WORDS is a multiple of 4 and acc starts on a 256-byte boundary
    const int gc = hd_cdiv((int64_t)n4, TB);
    hipLaunchKernelGGL(irp_clear_kernel, dim3(gc > 1024 ? 1024 : gc), dim3(TB), 0, s, (u32x4*)acc, n4);
  }
  // 16 bytes per lane: the passes that walk the flat plane when every plane starts on a 16-byte boundary (H*W a multiple of 4), the
  // stencil when every row does (W a multiple of 4); one float per lane otherwise
  const bool base16 = hd_aligned16(x) && hd_aligned16(out);
  const bool vec_plane = base16 && (P % 4) == 0, vec_row = base16 && (W % 4) == 0;
  const dim3 block(TB);
  const dim3 gh = grid_for(P, vec_plane ? 4 : 1, planes, MAXBX_HIST), gp = grid_for(P, vec_plane ? 4 : 1, planes, MAXBX);
  const dim3 gb = grid_for(P, vec_row ? 4 : 1, planes, MAXBX);
  const float* src = x;
  for (int k = 0; k < n_pass; ++k) {
    const Pass& ps = passes[k];
    float* dst = ((n_pass - 1 - k) & 1) ? tmp : out;
    uint32_t* a = acc + (size_t)k * acc_stage;
    if (ps.op == HD_IRP_STRETCH) {
      for (int level = 0; level < 4; ++level) {
        if (vec_plane) hipLaunchKernelGGL((irp_hist_kernel<4>), gh, block, 0, s, src, a, C, ps.mask, ps.pre, level, P);
        else hipLaunchKernelGGL((irp_hist_kernel<1>), gh, block, 0, s, src, a, C, ps.mask, ps.pre, level, P);
        hipLaunchKernelGGL(irp_resolve_kernel, dim3(planes), block, 0, s, a, C, ps.mask, level, P, q_out);
      }
    } else if (ps.op == HD_IRP_EQUALIZE) {
      if (vec_plane) hipLaunchKernelGGL((irp_hist_kernel<4>), gh, block, 0, s, src, a, C, ps.mask, ps.pre, -1, P);
      else hipLaunchKernelGGL((irp_hist_kernel<1>), gh, block, 0, s, src, a, C, ps.mask, ps.pre, -1, P);
    }
    if (ps.op == HD_IRP_BLUR) {
      if (vec_row) hipLaunchKernelGGL((irp_blur_kernel<4>), gb, block, 0, s, src, dst, C, ps.mask, ps.pre, ps.post, H, W);
      else hipLaunchKernelGGL((irp_blur_kernel<1>), gb, block, 0, s, src, dst, C, ps.mask, ps.pre, ps.post, H, W);
    } else {
      if (vec_plane) hipLaunchKernelGGL((irp_point_kernel<4>), gp, block, 0, s, src, dst, (const uint32_t*)a, C, ps.op, ps.mask, ps.pre, ps.post, P);
      else hipLaunchKernelGGL((irp_point_kernel<1>), gp, block, 0, s, src, dst, (const uint32_t*)a, C, ps.op, ps.mask, ps.pre, ps.post, P);
    }
    src = dst;
  }
  HD_CHECK_LAUNCH();
  return HD_OK;
}
