// Pixel reconstruction losses of the reference (src/losses/losses.py: torch.nn.MSELoss / L1Loss, weighted and summed into the
// total at train_hallucidet.py:173-176,209) as one streaming pass: both weighted terms, and optionally their gradient added into
// the caller's image gradient, for the hallucinated batch against the RGB batch and against the IR batch.
//   value   L = mean over N*3*H*W of v(h - t),            v(d) = d*d (mse) | |d| (l1)
//   grad    dL/dh = g(h - t),                             g(d) = 2d/n (mse) | sign(d)/n (l1), sign(0) = 0 as in torch
// The IR batch is either one plane per image (broadcast over the three channels, the layout the training step keeps) or three;
// its divisor is N*3*H*W either way (the reference averages over the three-channel view).
// One thread owns a position (n, o) of an image plane and walks the three channels there: the IR plane is read once, contiguously.
// Sums are two-stage (fixed block partials, then one block in index order): deterministic, no atomics.  Every mode evaluates the
// same per-element expressions in the same order, so value-only and gradient calls, eager and captured, agree bit for bit.
#include "hd_block.h"

namespace {

constexpr int LB = 256;        // threads per block
constexpr int NPART = 1024;    // most partial-sum blocks (part_ws holds 2 * NPART floats)

template <int KIND>
__device__ __forceinline__ float pix_value(float d) {
  return KIND == 0 ? d * d : fabsf(d);
}
// g(d) without its 1/n factor (folded into the per-launch coefficient): d (the 2 is in the coefficient) or sign(d)
template <int KIND>
__device__ __forceinline__ float pix_dir(float d) {
  return KIND == 0 ? d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
}

// positions q = n * PV + o, PV = H*W / V; channel c of image n is vector (n*3 + c)*PV + o of hall / rgb (and of a three-plane ir),
// vector n*PV + o of a one-plane ir.  part[b] = (sum v(h - rgb), sum v(h - ir)) of block b.
template <int KIND, bool IR3, bool GRAD, int V>
__global__ __launch_bounds__(LB) void pixel_loss_kernel(const float* __restrict__ hall, const float* __restrict__ rgb,
                                                        const float* __restrict__ ir, int64_t N, int64_t PV, float w_rgb, float w_ir,
                                                        float cn, const float* __restrict__ gs, float* __restrict__ dhall,
                                                        float* __restrict__ part) {
  __shared__ float sm[8];
  float sr = 0.f, si = 0.f;
  float coef = 0.f;
  if constexpr (GRAD) coef = *gs * cn;
  const int64_t total = N * PV;
  for (int64_t q = (int64_t)blockIdx.x * LB + threadIdx.x; q < total; q += (int64_t)gridDim.x * LB) {
    const int64_t n = q / PV;
    const int64_t o = q - n * PV;
    float iv[V];
    if constexpr (!IR3) hd_ldv<V>(ir + (n * PV + o) * V, iv);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t e = ((n * 3 + c) * PV + o) * V;
      float h[V], r[V];
      hd_ldv<V>(hall + e, h);
      hd_ldv<V>(rgb + e, r);
      if constexpr (IR3) hd_ldv<V>(ir + e, iv);
      float dg[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float dr = h[k] - r[k], di = h[k] - iv[k];
        sr += pix_value<KIND>(dr);
        si += pix_value<KIND>(di);
        if constexpr (GRAD) {
          const float t = w_rgb * pix_dir<KIND>(dr) + w_ir * pix_dir<KIND>(di);
          const float add = coef * t;
          dg[k] = add;
        }
      }
      if constexpr (GRAD) {
        float old[V];
        hd_ldv<V>(dhall + e, old);
#pragma unroll
        for (int k = 0; k < V; ++k) old[k] = old[k] + dg[k];
        hd_stv<V>(dhall + e, old);
      }
    }
  }
  hd_block_sum2<LB / 64>(sr, si, sm);
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2] = sr;
    part[blockIdx.x * 2 + 1] = si;
  }
}

// out[0] = w_rgb * (sum_rgb / n), out[1] = w_ir * (sum_ir / n), out[2] = (base + out[0]) + out[1] when base is given
__global__ __launch_bounds__(LB) void pixel_loss_finish_kernel(const float* __restrict__ part, int nb, float nf, float w_rgb, float w_ir,
                                                               const float* __restrict__ base, float* __restrict__ out) {
  __shared__ float sm[8];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < nb; i += LB) {
    a += part[i * 2];
    b += part[i * 2 + 1];
  }
  hd_block_sum2<LB / 64>(a, b, sm);
  if (threadIdx.x == 0) {
    const float lr = w_rgb * (a / nf), li = w_ir * (b / nf);
    out[0] = lr;
    out[1] = li;
    if (base) {
      const float t = *base + lr;
      out[2] = t + li;
    }
  }
}

template <int KIND, bool IR3, bool GRAD>
void launch_v(bool vec, int grid, hipStream_t s, const float* hall, const float* rgb, const float* ir, int64_t N, int64_t P, float w_rgb,
              float w_ir, float cn, const float* gs, float* dhall, float* part) {
  if (vec)
    hipLaunchKernelGGL((pixel_loss_kernel<KIND, IR3, GRAD, 4>), dim3(grid), dim3(LB), 0, s, hall, rgb, ir, N, P / 4, w_rgb, w_ir, cn, gs, dhall,
                       part);
  else
    hipLaunchKernelGGL((pixel_loss_kernel<KIND, IR3, GRAD, 1>), dim3(grid), dim3(LB), 0, s, hall, rgb, ir, N, P, w_rgb, w_ir, cn, gs, dhall, part);
}

template <int KIND>
void launch_k(bool ir3, bool grad, bool vec, int grid, hipStream_t s, const float* hall, const float* rgb, const float* ir, int64_t N, int64_t P,
              float w_rgb, float w_ir, float cn, const float* gs, float* dhall, float* part) {
  if (ir3) {
    if (grad) launch_v<KIND, true, true>(vec, grid, s, hall, rgb, ir, N, P, w_rgb, w_ir, cn, gs, dhall, part);
    else launch_v<KIND, true, false>(vec, grid, s, hall, rgb, ir, N, P, w_rgb, w_ir, cn, gs, dhall, part);
  } else {
    if (grad) launch_v<KIND, false, true>(vec, grid, s, hall, rgb, ir, N, P, w_rgb, w_ir, cn, gs, dhall, part);
    else launch_v<KIND, false, false>(vec, grid, s, hall, rgb, ir, N, P, w_rgb, w_ir, cn, gs, dhall, part);
  }
}

}  // namespace

extern "C" int hd_pixel_loss(const float* hall, const float* rgb, const float* ir, int N, int C, int H, int W, int ir_channels, float w_rgb,
                             float w_ir, int kind, const float* base_total, const float* gs, float* dhall, float* part_ws, float* out,
                             void* stream) {
  HD_CHECK_ARG(hall && rgb && ir && part_ws && out, "hd_pixel_loss: null pointer (hall, rgb, ir, part_ws and out are required)");
  HD_CHECK_ARG(C == 3, "hd_pixel_loss: C must be 3 (got %d)", C);
  HD_CHECK_ARG(ir_channels == 1 || ir_channels == 3, "hd_pixel_loss: ir_channels must be 1 or 3 (got %d)", ir_channels);
  HD_CHECK_ARG(kind == 0 || kind == 1, "hd_pixel_loss: kind must be 0 (mse) or 1 (l1) (got %d)", kind);
  HD_CHECK_ARG(N > 0 && H > 0 && W > 0, "hd_pixel_loss: bad shape N=%d H=%d W=%d", N, H, W);
  HD_CHECK_ARG(dhall == nullptr || gs != nullptr, "hd_pixel_loss: gradient mode (dhall) needs the device seed gs");
  const int64_t P = (int64_t)H * W;
  const int64_t n = (int64_t)N * 3 * P;
  // 16-byte accesses need every plane to start on a 16-byte boundary: H*W a multiple of 4 and 16-byte aligned bases
  const bool vec = (P % 4) == 0 && hd_aligned16(hall) && hd_aligned16(rgb) && hd_aligned16(ir) && hd_aligned16(dhall);
  const int64_t positions = (int64_t)N * (vec ? P / 4 : P);
  int64_t g = (positions + LB - 1) / LB;
  const int grid = (int)(g > NPART ? NPART : g);
  const float nf = (float)n;
  const float cn = (kind == 0 ? 2.f : 1.f) / nf;
  hipStream_t s = (hipStream_t)stream;
  const bool ir3 = ir_channels == 3, grad = dhall != nullptr;
  if (kind == 0)
    launch_k<0>(ir3, grad, vec, grid, s, hall, rgb, ir, N, P, w_rgb, w_ir, cn, gs, dhall, part_ws);
  else
    launch_k<1>(ir3, grad, vec, grid, s, hall, rgb, ir, N, P, w_rgb, w_ir, cn, gs, dhall, part_ws);
  hipLaunchKernelGGL(pixel_loss_finish_kernel, dim3(1), dim3(LB), 0, s, (const float*)part_ws, grid, nf, w_rgb, w_ir, base_total, out);
  HD_CHECK_LAUNCH();
  return HD_OK;
}
