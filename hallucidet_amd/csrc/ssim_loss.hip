// Structural reconstruction loss (--structural ssim): SSIM of Wang et al. 2004 with the constants of the common pytorch_msssim
// convention, for the hallucinated batch against the RGB batch and against the IR batch, as w * (1 - SSIM).
//   window  g[k] = exp(-(k-5)^2 / (2 * 1.5^2)) / sum, k = 0..10 (float64 on the host, stored fp32), separable, 'valid': maps are
//           Hm x Wm = (H-10) x (W-10);  data range 1, C1 = 1e-4, C2 = 9e-4
//   per channel, x = hallucinated, y = target:  mu_x = G*x, mu_y = G*y, mxx = G*x^2, myy = G*y^2, mxy = G*xy
//           A1 = 2 mu_x mu_y + C1, B1 = mu_x^2 + mu_y^2 + C1, A2 = 2 (mxy - mu_x mu_y) + C2, B2 = (mxx - mu_x^2) + (myy - mu_y^2) + C2
//           l = A1/B1, cs = A2/B2, S = l*cs;  SSIM = mean of S over N*3*Hm*Wm
//   grad    Pxx = -S/B2, Pxy = 2l/B2, Pm = cs (2/B1)(mu_y - l mu_x) + l (2/B2)(cs mu_x - mu_y) on the valid grid;
//           d sum S / d x_q = (G (*) Pm)_q + 2 x_q (G (*) Pxx)_q + y_q (G (*) Pxy)_q, (*) the full (transposed) correlation
// The IR batch is one plane per image (compared against each of the three channels; its own moments are filtered once per image) or
// three; the divisor is N*3*Hm*Wm either way.
//
// Two launches.  The forward kernel takes a TH x TW tile of the map: it stages x, r and i with their halo of 10 in LDS once, filters
// horizontally into LDS and vertically into registers (four vertically adjacent outputs per thread), and loops over the three
// channels; the x moments serve both terms.  In gradient mode it also writes the P maps, already weighted and merged where the
// filter is linear in them: c_r Pm_r + c_i Pm_i, c_r Pxx_r + c_i Pxx_i, c_r Pxy_r, c_i Pxy_i with c = -w / (N*3*Hm*Wm): four planes
// instead of six, stored in image coordinates (map position + 10) so that the gradient kernel's tiles start 16-byte aligned.
// The gradient kernel is the gather form: a TH x TW tile of dhall stages the four planes with a halo of 10 (zero outside the valid
// grid), filters them the same way and adds gs * (Fm + 2x Fxx + r Fxy_r + i Fxy_i): one writer per element, no atomics.
// Sums are two-stage (one partial pair per block, then one block in index order): deterministic, and the value-only and the
// gradient call evaluate the same expressions (the file is built without contraction), so their out bits agree.
#include <math.h>

#include "hd_block.h"

namespace {

constexpr int WIN = HD_SSIM_WINDOW;   // taps
constexpr int R = WIN - 1;            // halo
constexpr int TH = HD_SSIM_TILE_H;    // tile rows (map rows forward, image rows backward)
constexpr int TW = HD_SSIM_TILE_W;    // tile columns; one 32-lane half of a wave reads one row of the filtered tile: conflict-free
constexpr int IH = TH + R;            // staged rows
constexpr int IWV = (TW + R + 3) / 4; // staged 16-byte columns
constexpr int IWP = IWV * 4;          // staged row pitch (16-byte aligned rows)
constexpr int NT = 256;               // threads per block
constexpr int VR = 4;                 // vertically adjacent outputs per thread
constexpr int CG = TW / 4;            // 4-column groups of the horizontal pass
constexpr int MID = IH * TW;          // floats of one horizontally filtered map
static_assert(TW == 32 && TH * TW == NT * VR, "a thread owns a column of VR outputs; a 32-lane half owns a row");
static_assert(4 * (CG - 1) + 16 <= IWP, "the horizontal pass reads 16 staged floats per group");

struct Win {
  float g[WIN];
};

// dst[row][col] = plane[y0 + row][x0 + col] where lo <= y < H and lo <= x < W, else 0; rows 0..IH-1, columns 0..IWP-1.
// VEC: W % 4 == 0, x0 % 4 == 0 and a 16-byte aligned plane: one 16-byte load per four columns that lie inside the row.
template <bool VEC>
__device__ __forceinline__ void stage(const float* __restrict__ plane, int H, int W, int lo, int y0, int x0, float* __restrict__ dst) {
  for (int it = threadIdx.x; it < IH * IWV; it += NT) {
    const int row = it / IWV, v = it - row * IWV;
    const int gy = y0 + row, gx = x0 + 4 * v;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (gy >= lo && gy < H) {
      const float* p = plane + (int64_t)gy * W + gx;
      if (VEC && gx + 3 < W) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        t[0] = gx + 0 >= lo ? q.x : 0.f;
        t[1] = gx + 1 >= lo ? q.y : 0.f;
        t[2] = gx + 2 >= lo ? q.z : 0.f;
        t[3] = gx + 3 >= lo ? q.w : 0.f;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (gx + i >= lo && gx + i < W) t[i] = p[i];
      }
    }
    f32x4 o;
    o.x = t[0]; o.y = t[1]; o.z = t[2]; o.w = t[3];
    *reinterpret_cast<f32x4*>(dst + row * IWP + 4 * v) = o;
  }
}

// horizontal pass: mid[m][row][col] = sum_k g[k] * f(a, b)[m] at staged (row, col + k), rows 0..IH-1, columns 0..TW-1; a work item is
// four adjacent columns of one row (16 staged floats of each plane, 14 of them used)
template <int NM, class F>
__device__ __forceinline__ void hpass(const float* __restrict__ pa, const float* __restrict__ pb, float* __restrict__ mid, const Win& w, F f) {
  for (int it = threadIdx.x; it < IH * CG; it += NT) {
    const int row = it / CG, cg = it - row * CG;
    float a[16], b[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(pa + row * IWP + cg * 4 + q * 4);
      const f32x4 vb = *reinterpret_cast<const f32x4*>(pb + row * IWP + cg * 4 + q * 4);
      a[q * 4] = va.x; a[q * 4 + 1] = va.y; a[q * 4 + 2] = va.z; a[q * 4 + 3] = va.w;
      b[q * 4] = vb.x; b[q * 4 + 1] = vb.y; b[q * 4 + 2] = vb.z; b[q * 4 + 3] = vb.w;
    }
    float acc[NM][4];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[m][j] = 0.f;
#pragma unroll
    for (int e = 0; e < 4 + R; ++e) {
      float v[NM];
      f(a[e], b[e], v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = e - j;
        if (k >= 0 && k < WIN) {
#pragma unroll
          for (int m = 0; m < NM; ++m) acc[m][j] = __builtin_fmaf(w.g[k], v[m], acc[m][j]);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      f32x4 o;
      o.x = acc[m][0]; o.y = acc[m][1]; o.z = acc[m][2]; o.w = acc[m][3];
      *reinterpret_cast<f32x4*>(mid + m * MID + row * TW + cg * 4) = o;
    }
  }
}

// vertical pass: acc[m][j] = sum_k g[k] * mid[m][r0 + j + k][tx] for the thread's column tx and rows r0 .. r0 + VR - 1
template <int NM>
__device__ __forceinline__ void vpass(const float* __restrict__ mid, const Win& w, float (&acc)[NM][VR]) {
  const int tx = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * VR;
#pragma unroll
  for (int m = 0; m < NM; ++m) {
#pragma unroll
    for (int j = 0; j < VR; ++j) acc[m][j] = 0.f;
#pragma unroll
    for (int e = 0; e < VR + R; ++e) {
      const float v = mid[m * MID + (r0 + e) * TW + tx];
#pragma unroll
      for (int j = 0; j < VR; ++j) {
        const int k = e - j;
        if (k >= 0 && k < WIN) acc[m][j] = __builtin_fmaf(w.g[k], v, acc[m][j]);
      }
    }
  }
}

constexpr float SSIM_C1 = 1e-4f, SSIM_C2 = 9e-4f;

// S and, with GRAD, the three P maps at one position from the five moments
template <bool GRAD>
__device__ __forceinline__ float ssim_point(float mx, float my, float mxx, float myy, float mxy, float& pm, float& pxx, float& pxy) {
  const float mx2 = mx * mx, my2 = my * my, mxmy = mx * my;
  const float sx = mxx - mx2, sy = myy - my2, sxy = mxy - mxmy;
  const float A1 = 2.f * mxmy + SSIM_C1, B1 = (mx2 + my2) + SSIM_C1;
  const float A2 = 2.f * sxy + SSIM_C2, B2 = (sx + sy) + SSIM_C2;
  const float l = A1 / B1, cs = A2 / B2;
  const float S = l * cs;
  if constexpr (GRAD) {
    pxx = -S / B2;
    pxy = 2.f * l / B2;
    pm = cs * (2.f / B1) * (my - l * mx) + l * (2.f / B2) * (cs * mx - my);
  }
  return S;
}

// grid (tiles in x, tiles in y, N); part[block] = (sum S_rgb, sum S_ir) over the block's tile and the three channels.
// pws: four planes sets [4][N*3][H][W] in image coordinates (map position + R); maps: [2][N][3][Hm][Wm] or null.
template <bool IR3, bool GRAD, bool VEC>
__global__ __launch_bounds__(NT) void ssim_fwd_kernel(const float* __restrict__ hall, const float* __restrict__ rgb,
                                                      const float* __restrict__ ir, int N, int H, int W, Win w, float cr, float ci,
                                                      float* __restrict__ pws, float* __restrict__ maps, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_in[3][IH * IWP];
  __shared__ __attribute__((aligned(16))) float s_mid[5 * MID];
  __shared__ float s_red[8];
  const int Hm = H - R, Wm = W - R;
  const int n = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const int64_t P = (int64_t)H * W, Pm = (int64_t)Hm * Wm;
  const int tx = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * VR;
  float sr = 0.f, si = 0.f;
  float mi[2][VR];                               // G*i and G*i^2 of a one-plane IR: filtered once per image
  if constexpr (!IR3) stage<VEC>(ir + (int64_t)n * P, H, W, 0, y0, x0, s_in[2]);
  for (int c = 0; c < 3; ++c) {
    const int64_t pl = (int64_t)n * 3 + c;
    __syncthreads();                             // the previous channel's readers of s_in and s_mid are done
    stage<VEC>(hall + pl * P, H, W, 0, y0, x0, s_in[0]);
    stage<VEC>(rgb + pl * P, H, W, 0, y0, x0, s_in[1]);
    if constexpr (IR3) stage<VEC>(ir + pl * P, H, W, 0, y0, x0, s_in[2]);
    __syncthreads();
    hpass<5>(s_in[0], s_in[1], s_mid, w, [](float a, float b, float (&v)[5]) {
      v[0] = a; v[1] = a * a; v[2] = b; v[3] = b * b; v[4] = a * b;
    });
    __syncthreads();
    float m1[5][VR];                             // mu_x, mxx, mu_r, mrr, mxr
    vpass<5>(s_mid, w, m1);
    __syncthreads();
    const bool own = IR3 || c == 0;
    if (own)
      hpass<3>(s_in[0], s_in[2], s_mid, w, [](float a, float b, float (&v)[3]) { v[0] = a * b; v[1] = b; v[2] = b * b; });
    else
      hpass<1>(s_in[0], s_in[2], s_mid, w, [](float a, float b, float (&v)[1]) { v[0] = a * b; });
    __syncthreads();
    float mxi[1][VR];
    vpass<1>(s_mid, w, mxi);
    if (own) vpass<2>(s_mid + MID, w, mi);
#pragma unroll
    for (int j = 0; j < VR; ++j) {
      const int py = y0 + r0 + j, px = x0 + tx;
      if (py < Hm && px < Wm) {
        float pm_r = 0.f, pxx_r = 0.f, pxy_r = 0.f, pm_i = 0.f, pxx_i = 0.f, pxy_i = 0.f;
        const float Sr = ssim_point<GRAD>(m1[0][j], m1[2][j], m1[1][j], m1[3][j], m1[4][j], pm_r, pxx_r, pxy_r);
        const float Si = ssim_point<GRAD>(m1[0][j], mi[0][j], m1[1][j], mi[1][j], mxi[0][j], pm_i, pxx_i, pxy_i);
        sr += Sr;
        si += Si;
        if (maps) {
          const int64_t o = pl * Pm + (int64_t)py * Wm + px;
          maps[o] = Sr;
          maps[(int64_t)N * 3 * Pm + o] = Si;
        }
        if constexpr (GRAD) {
          const int64_t S4 = (int64_t)N * 3 * P;
          const int64_t o = pl * P + (int64_t)(py + R) * W + (px + R);
          pws[o] = cr * pm_r + ci * pm_i;
          pws[S4 + o] = cr * pxx_r + ci * pxx_i;
          pws[2 * S4 + o] = cr * pxy_r;
          pws[3 * S4 + o] = ci * pxy_i;
        }
      }
    }
  }
  hd_block_sum2<NT / 64>(sr, si, s_red);
  if (threadIdx.x == 0) {
    const int64_t b = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[b * 2] = sr;
    part[b * 2 + 1] = si;
  }
}

// out[3] = SSIM_rgb, out[4] = SSIM_ir, out[0] = w_rgb * (1 - out[3]), out[1] = w_ir * (1 - out[4]), out[2] = (base + out[0]) + out[1]
__global__ __launch_bounds__(NT) void ssim_finish_kernel(const float* __restrict__ part, int64_t nb, float nf, float w_rgb, float w_ir,
                                                         const float* __restrict__ base, float* __restrict__ out) {
  __shared__ float sm[8];
  float a = 0.f, b = 0.f;
  for (int64_t i = threadIdx.x; i < nb; i += NT) {
    a += part[i * 2];
    b += part[i * 2 + 1];
  }
  hd_block_sum2<NT / 64>(a, b, sm);
  if (threadIdx.x == 0) {
    const float qr = a / nf, qi = b / nf;
    const float lr = w_rgb * (1.f - qr), li = w_ir * (1.f - qi);
    out[0] = lr;
    out[1] = li;
    if (base) {
      const float t = *base + lr;
      out[2] = t + li;
    }
    out[3] = qr;
    out[4] = qi;
  }
}

// grid (tiles in x, tiles in y, N*3) over the image: dhall += gs * (Fm + 2x Fxx + r Fxy_r + i Fxy_i), F = the filtered planes of pws
template <bool IR3, bool VEC>
__global__ __launch_bounds__(NT) void ssim_bwd_kernel(const float* __restrict__ hall, const float* __restrict__ rgb,
                                                      const float* __restrict__ ir, int N, int H, int W, Win w,
                                                      const float* __restrict__ pws, const float* __restrict__ gs,
                                                      float* __restrict__ dhall) {
  __shared__ __attribute__((aligned(16))) float s_in[4][IH * IWP];
  __shared__ __attribute__((aligned(16))) float s_mid[4 * MID];
  const int64_t pl = blockIdx.z, P = (int64_t)H * W, S4 = (int64_t)N * 3 * P;
  const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const float seed = *gs;
  // image position q gathers map positions q - R .. q, i.e. rows y0 .. y0 + IH - 1 of the planes' image coordinates; below R is outside
#pragma unroll
  for (int k = 0; k < 4; ++k) stage<VEC>(pws + k * S4 + pl * P, H, W, R, y0, x0, s_in[k]);
  __syncthreads();
  auto both = [](float a, float b, float (&v)[2]) { v[0] = a; v[1] = b; };
  hpass<2>(s_in[0], s_in[1], s_mid, w, both);
  hpass<2>(s_in[2], s_in[3], s_mid + 2 * MID, w, both);
  __syncthreads();
  float F[4][VR];
  vpass<4>(s_mid, w, F);
  const int tx = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * VR;
  const int64_t n = pl / 3;
#pragma unroll
  for (int j = 0; j < VR; ++j) {
    const int qy = y0 + r0 + j, qx = x0 + tx;
    if (qy < H && qx < W) {
      const int64_t o = (int64_t)qy * W + qx, e = pl * P + o;
      const float x = hall[e], r = rgb[e], i = IR3 ? ir[e] : ir[n * P + o];
      const float d = ((F[0][j] + 2.f * x * F[1][j]) + r * F[2][j]) + i * F[3][j];
      dhall[e] = dhall[e] + seed * d;
    }
  }
}

inline int64_t part_floats(int N, int H, int W) {
  const int64_t nb = (int64_t)N * hd_cdiv(H - R, TH) * hd_cdiv(W - R, TW);
  return (2 * nb + 63) / 64 * 64;              // the P planes behind it start 16-byte aligned
}

Win make_window() {
  double g[WIN], s = 0.0;
  for (int k = 0; k < WIN; ++k) {
    const double d = k - (WIN - 1) / 2;
    g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    s += g[k];
  }
  Win w;
  for (int k = 0; k < WIN; ++k) w.g[k] = (float)(g[k] / s);
  return w;
}

template <bool IR3, bool GRAD>
void launch_fwd(bool vec, dim3 grid, hipStream_t s, const float* hall, const float* rgb, const float* ir, int N, int H, int W, const Win& w,
                float cr, float ci, float* pws, float* maps, float* part) {
  if (vec)
    hipLaunchKernelGGL((ssim_fwd_kernel<IR3, GRAD, true>), grid, dim3(NT), 0, s, hall, rgb, ir, N, H, W, w, cr, ci, pws, maps, part);
  else
    hipLaunchKernelGGL((ssim_fwd_kernel<IR3, GRAD, false>), grid, dim3(NT), 0, s, hall, rgb, ir, N, H, W, w, cr, ci, pws, maps, part);
}

template <bool IR3>
void launch_bwd(bool vec, dim3 grid, hipStream_t s, const float* hall, const float* rgb, const float* ir, int N, int H, int W, const Win& w,
                const float* pws, const float* gs, float* dhall) {
  if (vec)
    hipLaunchKernelGGL((ssim_bwd_kernel<IR3, true>), grid, dim3(NT), 0, s, hall, rgb, ir, N, H, W, w, pws, gs, dhall);
  else
    hipLaunchKernelGGL((ssim_bwd_kernel<IR3, false>), grid, dim3(NT), 0, s, hall, rgb, ir, N, H, W, w, pws, gs, dhall);
}

}  // namespace

extern "C" int64_t hd_ssim_loss_workspace(int N, int H, int W, int grad) {
  if (N <= 0 || N > 65535 / 3 || H < WIN || W < WIN) return -1;
  int64_t f = part_floats(N, H, W);
  if (grad) f += 4 * (int64_t)N * 3 * H * W;
  return f * (int64_t)sizeof(float);
}

extern "C" int hd_ssim_loss(const float* hall, const float* rgb, const float* ir, int N, int C, int H, int W, int ir_channels, float w_rgb,
                            float w_ir, const float* base_total, const float* gs, float* dhall, float* maps, void* ws, int64_t ws_bytes,
                            float* out, void* stream) {
  HD_CHECK_ARG(hall && rgb && ir && ws && out, "hd_ssim_loss: null pointer (hall, rgb, ir, ws and out are required)");
  HD_CHECK_ARG(C == 3, "hd_ssim_loss: C must be 3 (got %d)", C);
  HD_CHECK_ARG(ir_channels == 1 || ir_channels == 3, "hd_ssim_loss: ir_channels must be 1 or 3 (got %d)", ir_channels);
  HD_CHECK_ARG(N > 0 && N <= 65535 / 3, "hd_ssim_loss: N must be in 1..%d (got %d)", 65535 / 3, N);
  HD_CHECK_ARG(H >= WIN && W >= WIN, "hd_ssim_loss: H and W must be at least the window, %d (got H=%d W=%d)", WIN, H, W);
  HD_CHECK_ARG(dhall == nullptr || gs != nullptr, "hd_ssim_loss: gradient mode (dhall) needs the device seed gs");
  const bool grad = dhall != nullptr;
  const int64_t need = hd_ssim_loss_workspace(N, H, W, grad ? 1 : 0);
  HD_CHECK_ARG(ws_bytes >= need, "hd_ssim_loss: workspace too small (%lld bytes given, %lld needed)", (long long)ws_bytes, (long long)need);
  HD_CHECK_ARG(hd_aligned16(ws), "hd_ssim_loss: the workspace must be 16-byte aligned");
  static const Win w = make_window();
  const int Hm = H - R, Wm = W - R;
  const int64_t cnt = (int64_t)N * 3 * Hm * Wm;
  const float nf = (float)cnt;
  const float cr = -w_rgb / nf, ci = -w_ir / nf;
  float* part = static_cast<float*>(ws);
  float* pws = part + part_floats(N, H, W);
  // 16-byte accesses need every row of every plane on a 16-byte boundary: W a multiple of 4 and aligned bases (tiles start at
  // multiples of TW)
  const bool vec = (W % 4) == 0 && hd_aligned16(hall) && hd_aligned16(rgb) && hd_aligned16(ir);
  const bool ir3 = ir_channels == 3;
  hipStream_t s = (hipStream_t)stream;
  const dim3 gf(hd_cdiv(Wm, TW), hd_cdiv(Hm, TH), N);
  if (ir3) {
    if (grad) launch_fwd<true, true>(vec, gf, s, hall, rgb, ir, N, H, W, w, cr, ci, pws, maps, part);
    else launch_fwd<true, false>(vec, gf, s, hall, rgb, ir, N, H, W, w, cr, ci, pws, maps, part);
  } else {
    if (grad) launch_fwd<false, true>(vec, gf, s, hall, rgb, ir, N, H, W, w, cr, ci, pws, maps, part);
    else launch_fwd<false, false>(vec, gf, s, hall, rgb, ir, N, H, W, w, cr, ci, pws, maps, part);
  }
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(NT), 0, s, (const float*)part, (int64_t)gf.x * gf.y * gf.z, nf, w_rgb, w_ir,
                     base_total, out);
  if (grad) {
    const dim3 gb(hd_cdiv(W, TW), hd_cdiv(H, TH), N * 3);
    if (ir3) launch_bwd<true>(vec, gb, s, hall, rgb, ir, N, H, W, w, pws, gs, dhall);
    else launch_bwd<false>(vec, gb, s, hall, rgb, ir, N, H, W, w, pws, gs, dhall);
  }
  HD_CHECK_LAUNCH();
  return HD_OK;
}
