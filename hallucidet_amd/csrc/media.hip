// Detection media panels: a planar fp32 batch rendered as ONE uint8 HWC image (torchvision's make_grid layout), either quantised as
// save_image does (raw panels) or min-max normalised per image and channel with ground-truth and detection outlines drawn over it
// (the reference's Utils.plot_each_image / show_bbox, src/utils/utils.py:137-297, without the text labels).
//   pass 1 (normalise only)  block partials of every plane's min / max: B blocks per plane, part[plane][b] = (mn, mx)
//   pass 2                   one unit = one canvas row x a group of G grid cells.  The unit's bytes are built in LDS at the same
//                            address mod 16 as their place in the canvas: the block combines the cells' partials (integer LDS
//                            atomics on the ordered image of the float bits: order-free), reads every fp32 value once (16 bytes per
//                            lane on the wide path), writes its byte at the HWC position, paints the outlines that cross this image
//                            row (ground truths, barrier, detections), then stores the row in 16-byte pieces (single bytes only up to
//                            the first and after the last 16-byte boundary).  Padding rows are stored as zeros directly.
// Every output byte has one writer and the painting order is fixed by barriers: the same bytes from run to run.
#include "hd_block.h"
#include <math.h>

namespace {

constexpr int LB = 256;                   // threads per block
constexpr int MMB = 32;                   // most min/max partial blocks per plane
constexpr int MM_FLOATS = 16384;          // floats of a plane per partial block, at least
constexpr int RUNS = 1024;                // (cell, box) pairs examined per painting round = capacity of the horizontal-run list
constexpr int LDS_DATA_MAX = 40 * 1024;   // most bytes of one unit (9 cells at W = 1499)
constexpr int UNIT_MIN_BYTES = 4096;      // a cell group is not split below this many bytes per unit
constexpr int MAX_BLOCKS = 2048;
constexpr int MAX_IMAGES = 16384;         // 3 * N is a grid dimension of the min/max pass

// grid (B, N * PC): block b of plane (n, c) reduces floats [b * chunk, min((b + 1) * chunk, HW)) of it; chunk % 4 == 0
template <int V>
__global__ __launch_bounds__(LB) void media_minmax_kernel(const float* __restrict__ x, int64_t sn, int64_t sc, int PC, int64_t HW,
                                                          int64_t chunk, float2* __restrict__ part) {
  __shared__ float sm[8];
  const int plane = blockIdx.y;
  const int n = plane / PC, c = plane - n * PC;
  const float* p = x + n * sn + c * sc;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < HW ? lo + chunk : HW;
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
  for (int64_t i = lo + (int64_t)threadIdx.x * V; i < hi; i += (int64_t)LB * V) {
    float v[V];
    hd_ldv<V>(p + i, v);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      mn = fminf(mn, v[e]);
      mx = fmaxf(mx, v[e]);
    }
  }
  hd_wave_reduce2(mn, HdMin(), mx, HdMax());
  const float mm[2] = {mn, mx};
  hd_block_put(mm, sm);
  if (threadIdx.x == 0) {
    mn = fminf(fminf(sm[0], sm[2]), fminf(sm[4], sm[6]));
    mx = fmaxf(fmaxf(sm[1], sm[3]), fmaxf(sm[5], sm[7]));
    part[(int64_t)plane * gridDim.x + blockIdx.x] = make_float2(mn, mx);
  }
}

struct RenderArgs {
  const float* x;
  int64_t sn, sc;
  int N, H, W, xmaps, pad, CW, CH, G, ngroups;
  const float2* part;          // [N * PC][B]
  int PC, B;
  const void* db;              // detections [N][P][4] fp32 / fp64
  int db64;
  const float* ds;
  const int* dc;
  int P;
  float thr;
  const double* gb;            // ground truths [N][Q][4]
  const int* gc;
  int Q;
  uint8_t* canvas;
  int data_bytes, key_words;   // LDS carve: data | mn keys | mx keys | 2 counters (+2 pad) | runs
};

__device__ __forceinline__ int trunc_corner(double v) {
  v = v > -1048576.0 ? v : -1048576.0;      // far outside any image either way; NaN -> outside
  v = v < 1048576.0 ? v : 1048576.0;
  return (int)v;
}

__device__ __forceinline__ void paint(unsigned char* px, int pass) {
  px[0] = 255;
  px[1] = pass == 0 ? 255 : 0;
  px[2] = 0;
}

// nbytes bytes from LDS `src` (nullptr: zeros) to `gp`; src and gp are congruent mod 16
__device__ __forceinline__ void store_row(uint8_t* gp, const unsigned char* src, int nbytes) {
  const int tid = threadIdx.x;
  const int mis = (int)(reinterpret_cast<uintptr_t>(gp) & 15);
  const int head = ((16 - mis) & 15) < nbytes ? ((16 - mis) & 15) : nbytes;
  if (tid < head) gp[tid] = src ? src[tid] : (unsigned char)0;
  const int nv = (nbytes - head) >> 4;
  for (int i = tid; i < nv; i += LB) {
    u32x4 t = {0u, 0u, 0u, 0u};
    if (src) t = *reinterpret_cast<const u32x4*>(src + head + 16 * i);
    *reinterpret_cast<u32x4*>(gp + head + 16 * i) = t;
  }
  const int t0 = head + 16 * nv;
  if (tid < nbytes - t0) gp[t0 + tid] = src ? src[t0 + tid] : (unsigned char)0;
}

template <int V, int MODE>
__global__ __launch_bounds__(LB) void media_render_kernel(RenderArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* smn = reinterpret_cast<uint32_t*>(smem + a.data_bytes);
  uint32_t* smx = smn + a.key_words;
  int* cnt = reinterpret_cast<int*>(smx + a.key_words);
  uint32_t* runs = reinterpret_cast<uint32_t*>(cnt + 4);
  const int tid = threadIdx.x;
  const int pitch = a.W + a.pad, pitch_y = a.H + a.pad;
  const int units = a.CH * a.ngroups;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int r = u / a.ngroups, g = u - r * a.ngroups;
    const int j0 = g * a.G;
    const int cells = a.G < a.xmaps - j0 ? a.G : a.xmaps - j0;
    const int tailpad = g == a.ngroups - 1 ? a.pad : 0;        // the canvas row's closing padding belongs to its last group
    const int nbytes = (cells * pitch + tailpad) * 3;
    uint8_t* gp = a.canvas + ((int64_t)r * a.CW + (int64_t)j0 * pitch) * 3;
    const int rr = r - a.pad;
    int gy = -1, y = 0;
    if (rr >= 0) {
      gy = rr / pitch_y;
      y = rr - gy * pitch_y;
      if (y >= a.H) gy = -1;
    }
    if (gy < 0) {                                              // a padding row (uniform over the block)
      store_row(gp, nullptr, nbytes);
      continue;
    }
    unsigned char* data = smem + (reinterpret_cast<uintptr_t>(gp) & 15);
    // the padding columns in front of every cell and behind the last one
    const int padb = a.pad * 3;
    for (int i = tid; i < (cells + (tailpad ? 1 : 0)) * padb; i += LB) {
      const int jj = i / padb;
      data[jj * pitch * 3 + (i - jj * padb)] = 0;
    }
    if constexpr (MODE == HD_MEDIA_NORMALISE) {
      for (int i = tid; i < cells * 3; i += LB) {
        smn[i] = 0xffffffffu;
        smx[i] = 0u;
      }
      if (tid == 0) cnt[0] = cnt[1] = 0;
      __syncthreads();
      const int per = a.PC * a.B;
      for (int i = tid; i < cells * per; i += LB) {
        const int j = i / per, rem = i - j * per;
        const int c = rem / a.B, b = rem - c * a.B;
        const int k = gy * a.xmaps + j0 + j;
        if (k < a.N) {
          const float2 m = a.part[((int64_t)k * a.PC + c) * a.B + b];
          atomicMin(&smn[j * 3 + c], hd_float_key(m.x));
          atomicMax(&smx[j * 3 + c], hd_float_key(m.y));
        }
      }
      __syncthreads();
    }
    // pixels
    const int WV = a.W / V;
    const int items = cells * WV;
#pragma unroll 2
    for (int idx = tid; idx < items; idx += LB) {
      const int j = idx / WV, xv = idx - j * WV;
      const int k = gy * a.xmaps + j0 + j;
      unsigned char* d = data + (j * pitch + a.pad + xv * V) * 3;
      if (k >= a.N) {                                          // an empty cell of the last grid row
#pragma unroll
        for (int e = 0; e < 3 * V; ++e) d[e] = 0;
        continue;
      }
      const float* p = a.x + (int64_t)k * a.sn + (int64_t)y * a.W + xv * V;
      unsigned char bt[V];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c == 0 || a.sc != 0) {                             // a stride-0 channel view: one load, one conversion
          float v[V];
          hd_ldv<V>(p + c * a.sc, v);
          if constexpr (MODE == HD_MEDIA_NORMALISE) {
            const int kc = j * 3 + (a.PC == 3 ? c : 0);
            const float mn = hd_key_float(smn[kc]), mx = hd_key_float(smx[kc]);
            const float rng = mx - mn;
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const float t = v[e] - mn;
              const float q = rng != 0.f ? t / rng : 0.f;
              bt[e] = (unsigned char)(int)(q * 255.f);
            }
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
              float t = v[e] * 255.f;
              t = t + 0.5f;
              t = fminf(fmaxf(t, 0.f), 255.f);
              bt[e] = (unsigned char)(int)t;
            }
          }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) d[e * 3 + c] = bt[e];
      }
    }
    __syncthreads();
    if constexpr (MODE == HD_MEDIA_NORMALISE) {
      int round = 0;
      for (int pass = 0; pass < 2; ++pass) {                   // 0: ground truths, yellow; 1: detections above the threshold, red
        const int M = pass == 0 ? a.Q : a.P;
        const int total = cells * M;
        for (int base = 0; base < total; base += RUNS, ++round) {
          int* mycnt = cnt + (round & 1);
          if (tid == 0) cnt[(round + 1) & 1] = 0;
          const int end = base + RUNS < total ? base + RUNS : total;
          for (int i = base + tid; i < end; i += LB) {
            const int j = i / M, b = i - j * M;
            const int k = gy * a.xmaps + j0 + j;
            if (k >= a.N) continue;
            int count = pass == 0 ? a.gc[k] : a.dc[k];
            count = count < M ? count : M;
            if (b >= count) continue;
            const int64_t row = (int64_t)k * M + b;
            int x1, y1, x2, y2;
            if (pass == 0 || a.db64) {
              const double* q = (pass == 0 ? a.gb : static_cast<const double*>(a.db)) + row * 4;
              if (pass == 1 && !(a.ds[row] > a.thr)) continue;
              x1 = trunc_corner(q[0]); y1 = trunc_corner(q[1]); x2 = trunc_corner(q[2]); y2 = trunc_corner(q[3]);
            } else {
              if (!(a.ds[row] > a.thr)) continue;
              const float* q = static_cast<const float*>(a.db) + row * 4;
              x1 = trunc_corner(q[0]); y1 = trunc_corner(q[1]); x2 = trunc_corner(q[2]); y2 = trunc_corner(q[3]);
            }
            unsigned char* cell = data + (j * pitch + a.pad) * 3;
            const int ylo = y1 < y2 ? y1 : y2, yhi = y1 < y2 ? y2 : y1;
            if (y >= ylo && y <= yhi) {                        // the two vertical lines
              if (x1 >= 0 && x1 < a.W) paint(cell + x1 * 3, pass);
              if (x2 >= 0 && x2 < a.W) paint(cell + x2 * 3, pass);
            }
            if (y == y1 || y == y2) {                          // a horizontal line: painted by the whole block below
              int xa = x1 < x2 ? x1 : x2, xb = x1 < x2 ? x2 : x1;
              xa = xa > 0 ? xa : 0;
              xb = xb < a.W - 1 ? xb : a.W - 1;
              if (xa <= xb) runs[atomicAdd(mycnt, 1)] = (uint32_t)j << 22 | (uint32_t)xa << 11 | (uint32_t)xb;
            }
          }
          __syncthreads();
          const int n = *mycnt;
          for (int e = 0; e < n; ++e) {
            const uint32_t rn = runs[e];
            unsigned char* cell = data + ((int)(rn >> 22) * pitch + a.pad) * 3;
            const int xb = (int)(rn & 2047u);
            for (int xx = (int)((rn >> 11) & 2047u) + tid; xx <= xb; xx += LB) paint(cell + xx * 3, pass);
          }
          __syncthreads();
        }
      }
    }
    store_row(gp, data, nbytes);
    __syncthreads();                                           // the next unit rebuilds the LDS row
  }
}


}  // namespace

extern "C" int64_t hd_media_ws_bytes(int N) {
  if (N < 1 || N > MAX_IMAGES) return HD_E_ARG;
  return (int64_t)N * 3 * MMB * (int64_t)sizeof(float2);
}

extern "C" int hd_media_render(const float* x, int64_t stride_n, int64_t stride_c, int N, int H, int W, int nrow, int mode,
                               const void* det_boxes, int det_boxes_f64, const float* det_scores, const int32_t* det_count, int P,
                               float threshold, const double* gt_boxes, const int32_t* gt_count, int Q, uint8_t* canvas, void* ws,
                               void* stream) {
  HD_CHECK_ARG(x && canvas, "hd_media_render: null pointer (x and canvas are required)");
  HD_CHECK_ARG(mode == HD_MEDIA_QUANTISE || mode == HD_MEDIA_NORMALISE, "hd_media_render: mode must be 0 (quantise) or 1 (normalise) (got %d)",
               mode);
  HD_CHECK_ARG(N >= 1 && N <= MAX_IMAGES && H >= 1 && W >= 1 && nrow >= 1, "hd_media_render: bad shape N=%d H=%d W=%d nrow=%d", N, H, W, nrow);
  HD_CHECK_ARG(H <= HD_MEDIA_MAX_SIDE && W <= HD_MEDIA_MAX_SIDE,
               "hd_media_render: max(H, W) must be <= %d (outline thickness 2 is not built) (got %d x %d)", HD_MEDIA_MAX_SIDE, H, W);
  HD_CHECK_ARG(stride_n >= 0 && stride_c >= 0, "hd_media_render: negative stride");
  const bool norm = mode == HD_MEDIA_NORMALISE;
  if (!norm) P = Q = 0;
  HD_CHECK_ARG(P >= 0 && P <= HD_MEDIA_DET_CAP, "hd_media_render: P = %d detections per image, the cap is %d", P, HD_MEDIA_DET_CAP);
  HD_CHECK_ARG(Q >= 0 && Q <= HD_MEDIA_GT_CAP, "hd_media_render: Q = %d ground truths per image, the cap is %d", Q, HD_MEDIA_GT_CAP);
  HD_CHECK_ARG(!norm || ws, "hd_media_render: normalise mode needs the workspace");
  HD_CHECK_ARG(P == 0 || (det_boxes && det_scores && det_count), "hd_media_render: P > 0 needs det_boxes, det_scores and det_count");
  HD_CHECK_ARG(Q == 0 || (gt_boxes && gt_count), "hd_media_render: Q > 0 needs gt_boxes and gt_count");
  hipStream_t s = (hipStream_t)stream;
  RenderArgs a;
  a.x = x; a.sn = stride_n; a.sc = stride_c;
  a.N = N; a.H = H; a.W = W;
  a.xmaps = nrow < N ? nrow : N;
  const int ymaps = (N + a.xmaps - 1) / a.xmaps;
  a.pad = N == 1 ? 0 : 2;
  a.CW = a.xmaps * (W + a.pad) + a.pad;
  a.CH = ymaps * (H + a.pad) + a.pad;
  // cells per unit: what fits the LDS row; halved while the grid is short of ~1024 units and the halves stay >= UNIT_MIN_BYTES
  const int cell_bytes = (W + a.pad) * 3;
  int G = (LDS_DATA_MAX - 32) / cell_bytes;
  G = G < a.xmaps ? G : a.xmaps;
  G = G < 1023 ? G : 1023;
  while (G > 1 && (int64_t)a.CH * ((a.xmaps + G - 1) / G) < 1024 && ((G + 1) / 2) * cell_bytes >= UNIT_MIN_BYTES) G = (G + 1) / 2;
  a.G = G;
  a.ngroups = (a.xmaps + G - 1) / G;
  a.data_bytes = (16 + G * cell_bytes + a.pad * 3 + 15) & ~15;
  a.key_words = (G * 3 + 3) & ~3;
  const size_t lds = (size_t)a.data_bytes + (size_t)a.key_words * 8 + 16 + RUNS * 4;
  a.PC = stride_c == 0 ? 1 : 3;
  const int64_t HW = (int64_t)H * W;
  int B = (int)(HW / MM_FLOATS);
  B = B < 1 ? 1 : (B > MMB ? MMB : B);
  a.B = B;
  a.part = static_cast<const float2*>(ws);
  a.db = det_boxes; a.db64 = det_boxes_f64; a.ds = det_scores; a.dc = det_count; a.P = P; a.thr = threshold;
  a.gb = gt_boxes; a.gc = gt_count; a.Q = Q;
  a.canvas = canvas;
  // 16-byte loads need every image row to start on a 16-byte boundary
  const bool vec = (W % 4) == 0 && (stride_n % 4) == 0 && (stride_c % 4) == 0 && hd_aligned16(x);
  if (norm) {
    const int64_t chunk = (((HW + B - 1) / B) + 3) & ~(int64_t)3;
    const dim3 grid(B, N * a.PC);
    if (vec)
      hipLaunchKernelGGL((media_minmax_kernel<4>), grid, dim3(LB), 0, s, x, stride_n, stride_c, a.PC, HW, chunk, static_cast<float2*>(ws));
    else
      hipLaunchKernelGGL((media_minmax_kernel<1>), grid, dim3(LB), 0, s, x, stride_n, stride_c, a.PC, HW, chunk, static_cast<float2*>(ws));
    HD_CHECK_LAUNCH();
  }
  const int64_t units = (int64_t)a.CH * a.ngroups;
  const int grid = (int)(units < MAX_BLOCKS ? units : MAX_BLOCKS);
  if (norm) {
    if (vec) hipLaunchKernelGGL((media_render_kernel<4, HD_MEDIA_NORMALISE>), dim3(grid), dim3(LB), lds, s, a);
    else hipLaunchKernelGGL((media_render_kernel<1, HD_MEDIA_NORMALISE>), dim3(grid), dim3(LB), lds, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((media_render_kernel<4, HD_MEDIA_QUANTISE>), dim3(grid), dim3(LB), lds, s, a);
    else hipLaunchKernelGGL((media_render_kernel<1, HD_MEDIA_QUANTISE>), dim3(grid), dim3(LB), lds, s, a);
  }
  HD_CHECK_LAUNCH();
  return HD_OK;
}
