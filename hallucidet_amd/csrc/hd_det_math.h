// The detector's fp32 formulas whose rounding is contractual: the tests pin them, operation by operation, to ATen's and torchvision's
// element-wise code, and several kernels (loss forward / backward, target assignment, sampling tails, NMS) must agree on them bit for
// bit.  One definition each; a change here changes every user at once.
// Every product, sum and quotient below is ONE IEEE operation.  The library is built with -ffp-contract=off, which is all these
// functions need; each body repeats that as a pragma, so the header does not depend on a `#pragma clang fp contract(off)` in the
// including file (detection.hip has one, losses.hip and fcos.hip do not) or on the order of includes.
#pragma once
#include "hd_common.h"

// torch.sigmoid as ATen evaluates it in fp32
__device__ __forceinline__ float hd_sigmoid(float x) {
#pragma clang fp contract(off)
  return 1.f / (1.f + expf(-x));
}

// ATen's binary_cross_entropy_with_logits, per element: (1 - t) * x + m + log(exp(-m) + exp(-x - m)), m = max(-x, 0)
__device__ __forceinline__ float hd_bce_logits(float x, float t) {
#pragma clang fp contract(off)
  const float m = fmaxf(-x, 0.f);
  return (1.f - t) * x + m + logf(expf(-m) + expf(-x - m));
}

// torchvision.ops.sigmoid_focal_loss [EXT] (reference src/utils/eval_forward_retinanet.py:22-50):
//   focal(x, t) = alpha_t * bce(x, t) * (1 - p_t)^gamma,  p = sigmoid(x), p_t = t ? p : 1 - p,  alpha < 0: no alpha factor
// ce is the target-independent part of the BCE: bce(x, t) = (1 - t) * x + ce, and for the 0 / 1 targets used here x is added AFTER the
// sum inside ce -- not hd_bce_logits' association.
struct FocalT {
  float ce, p;
};
__device__ __forceinline__ FocalT focal_terms(float x) {
#pragma clang fp contract(off)
  FocalT r;
  r.p = hd_sigmoid(x);
  const float m = fmaxf(-x, 0.f);
  r.ce = m + logf(expf(-m) + expf(-x - m));
  return r;
}
__device__ __forceinline__ float focal_value(float x, bool t, float alpha, float gamma) {
#pragma clang fp contract(off)
  const FocalT f = focal_terms(x);
  const float ce = t ? f.ce : x + f.ce;
  const float pt = t ? f.p : 1.f - f.p;
  const float w = gamma == 2.f ? (1.f - pt) * (1.f - pt) : powf(1.f - pt, gamma);
  float l = ce * w;
  if (alpha >= 0.f) l *= t ? alpha : 1.f - alpha;
  return l;
}
__device__ __forceinline__ float focal_grad(float x, bool t, float alpha, float gamma) {
#pragma clang fp contract(off)
  const FocalT f = focal_terms(x);
  const float p = f.p, q = 1.f - f.p;
  float g;
  if (t) {
    const float w = gamma == 2.f ? q * q : powf(q, gamma);
    g = w * (-gamma * p * f.ce - q);
  } else {
    const float w = gamma == 2.f ? p * p : powf(p, gamma);
    g = w * (p + gamma * q * (x + f.ce));
  }
  if (alpha >= 0.f) g *= t ? alpha : 1.f - alpha;
  return g;
}

// ATen's smooth_l1_loss(beta) per element and its derivative: 0.5 * d * d / beta below beta, |d| - 0.5 * beta above
__device__ __forceinline__ float smooth_l1(float d, float beta) {
#pragma clang fp contract(off)
  const float z = fabsf(d);
  return z < beta ? 0.5f * z * z / beta : z - 0.5f * beta;
}
__device__ __forceinline__ float smooth_l1_grad(float d, float beta) { return d < -beta ? -1.f : (d > beta ? 1.f : d / beta); }

// torchvision BoxCoder.encode_single [EXT]: the regression target of box g (x1, y1, x2, y2) against the anchor / proposal a.
// Centres are x + 0.5 * w; the weight multiplies the centre difference BEFORE the division by the anchor's size.
__device__ __forceinline__ float4 encode_box(float4 g, float4 a, float wx, float wy, float ww, float wh) {
#pragma clang fp contract(off)
  const float ew = a.z - a.x, eh = a.w - a.y, ecx = a.x + 0.5f * ew, ecy = a.y + 0.5f * eh;
  const float gw = g.z - g.x, gh = g.w - g.y, gcx = g.x + 0.5f * gw, gcy = g.y + 0.5f * gh;
  return make_float4(wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * logf(gw / ew), wh * logf(gh / eh));
}

// torchvision.ops.box_iou [EXT] for one pair of (x1, y1, x2, y2) boxes, in the scalar CPU oracle's operation order
__device__ __forceinline__ float box_iou_dev(const float* a, const float* b) {
#pragma clang fp contract(off)
  float area_a = (a[2] - a[0]) * (a[3] - a[1]);
  float area_b = (b[2] - b[0]) * (b[3] - b[1]);
  float xx1 = fmaxf(a[0], b[0]), yy1 = fmaxf(a[1], b[1]);
  float xx2 = fminf(a[2], b[2]), yy2 = fminf(a[3], b[3]);
  float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  float inter = w * h;
  return inter / (area_a + area_b - inter);
}
