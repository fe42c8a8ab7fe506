// Streaming kernels for the detector's THIN 1x1 problems: a handful of output channels in the forward direction (RPNHead.cls_logits /
// bbox_pred: 256 -> 3 and 12; FastRCNNPredictor.cls_score / bbox_pred: 1024 -> 2 and 8 [EXT], reached from
// src/utils/eval_forward_fasterrcnn.py), or a handful of reduction channels in their data gradients (8 / 16 -> 256 / 1024).
//
// Why a third GEMM path.  In the 4-wave implicit-GEMM family these problems run on 32- and 64-wide MFMA tiles whose columns are mostly
// padding: the time of a block is its set-up, LDS staging and epilogue, not its K loop (4096 x 1024 -> 8: 21 us against 1.1 us for its
// bytes), the two heads of a pair each read the shared input, and the gradient pair writes its sum, reads it back as `res` and writes it
// again behind two pad-and-cast launches.  Both kernels here are LDS-free: MFMA fragments are loaded straight from global memory in the
// layout v_mfma_f32_32x32x16_f16 wants -- lane -> row lane & 31, the 8 consecutive k at 16 ks + 8 (lane >> 5) = one 16-byte load; the
// eight loads of a 64-deep stretch cover each row's 128-byte line exactly once.  A wave owns 32 GEMM rows and the full K chain of its outputs.
//
// Exactness.  One fp32 chain per output, the same instruction over ascending 16-deep k chunks (k = 64 kt + 16 ks + 8 h + j) as the
// implicit-GEMM family; chunks that are entirely padding are skipped (they add exact zeros: an fp32 chain that starts at +0 never
// holds -0).  The epilogues repeat conv_epilogue.h's operations in its order, so every output is bit-identical to that family's
// (tests/test_thin_gemm_gpu.py).
//
//   thin-N forward     y_a[M][ca], y_b[M][cb] = act(x[M][K] . Wa^T + bias_a), act(x . Wb^T + bias_b), fp32: the one or two heads that share
//                      x sit in ONE MFMA A operand (rows 0 .. ca-1 and cap .. cap+cb-1, cap = ca rounded up to 4, cap + cbp <= 32), x is the
//                      B operand and is read once; a lane then holds 4 consecutive channels of one row per register group.
//   thin-K pair        dx[M][C] = f16( mask( f16(gA . WdA) + gB . WdB ) ): the gradients are the A operand (rows = pixels), the weights the
//                      B operand with column c of MFMA j standing for channel cbase + NJ c + j, so the NJ accumulators of a lane hold NJ
//                      CONSECUTIVE channels of a pixel and the 32 lanes of a half-wave one contiguous run of 32 NJ channels: mask loads and
//                      stores are 8 bytes per lane, 256 contiguous bytes per pixel (NJ = 4), with all 16 mask loads of a 32-pixel group
//                      requested before the first MFMA.  The weights of a pass stay in registers over the wave's pixel groups.
#include "hd_common.h"
#include "conv_params.h"

namespace {

// ------------------------------------------------------------------ thin-N forward
struct ThinFwdP {
  const f16* x;
  const f16* wa;
  const f16* wb;        // null: a single head
  const float* ba;
  const float* bb;
  float* ya;
  float* yb;
  int M, K, ca, cb, cap, act;
};
struct ThinFwdTab {
  ThinFwdP p[HD_CONV_MULTI_MAX];
  int first[HD_CONV_MULTI_MAX + 1];     // blocks [first[i], first[i+1]) belong to problem i
  int n;
};

__device__ __forceinline__ f16x8 ld8g(const f16* q) { return *reinterpret_cast<const f16x8*>(q); }

// RG: 32-row groups per wave (the weight fragments are loaded once per wave and K step), U: K steps whose loads are requested together
template <int RG, int U>
__global__ __launch_bounds__(64) void thin_fwd_kernel(ThinFwdTab t) {
  int pi = 0;
  for (int i = 1; i < t.n; ++i)
    if ((int)blockIdx.x >= t.first[i]) pi = i;
  const ThinFwdP p = t.p[pi];
  const int lane = threadIdx.x, frow = lane & 31, fh = lane >> 5;
  const int row0 = ((int)blockIdx.x - t.first[pi]) * (32 * RG);
  const int M = p.M, K = p.K;

  // rows of the A operand that belong to no head, and rows of x past M, read a valid row: MFMA rows and columns do not mix, and
  // what they produce is never stored
  const bool in_b = frow >= p.cap && frow < p.cap + p.cb;
  const f16* wrow = frow < p.ca ? p.wa + (size_t)frow * K : (in_b ? p.wb + (size_t)(frow - p.cap) * K : p.wa);
  const f16* xrow[RG];
#pragma unroll
  for (int g = 0; g < RG; ++g) {
    const int m = row0 + 32 * g + frow;
    xrow[g] = p.x + (size_t)(m < M ? m : M - 1) * K;
  }

  f32x16 acc[RG];
#pragma unroll
  for (int g = 0; g < RG; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;

  const int nfull = K >> 4;          // K steps without a padded half
  int ks = 0;
  for (; ks + U <= nfull; ks += U) {
    f16x8 wf[U], xf[U][RG];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k0 = (ks + u) * 16 + 8 * fh;
      wf[u] = ld8g(wrow + k0);
#pragma unroll
      for (int g = 0; g < RG; ++g) xf[u][g] = ld8g(xrow[g] + k0);
    }
    // all U steps' loads are requested before the first MFMA waits (left alone the scheduler pairs each load with its MFMA: one
    // memory latency per K step)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int g = 0; g < RG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[u], xf[u][g], acc[g], 0, 0, 0);
  }
  for (; ks * 16 < K; ++ks) {        // the remaining steps one by one; the half past K (K % 16 == 8) is zero in both operands
    const int k0 = ks * 16 + 8 * fh;
    const bool kv = k0 < K;
    const int kc = kv ? k0 : K - 8;
    f16x8 wf = ld8g(wrow + kc);
    f16x8 xf[RG];
#pragma unroll
    for (int g = 0; g < RG; ++g) xf[g] = ld8g(xrow[g] + kc);
#pragma unroll
    for (int j = 0; j < 8; ++j) wf[j] = kv ? wf[j] : (f16)0.f;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
#pragma unroll
      for (int j = 0; j < 8; ++j) xf[g][j] = kv ? xf[g][j] : (f16)0.f;
      acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xf[g], acc[g], 0, 0, 0);
    }
  }

  // acc[g][4 q + i] = A-operand row 8 q + 4 fh + i of GEMM row row0 + 32 g + frow: four consecutive channels of one head
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int sb = 8 * q + 4 * fh;
    const bool a_side = sb < p.cap;
    const int c0 = a_side ? sb : sb - p.cap;
    const int cout = a_side ? p.ca : p.cb;
    if (c0 >= cout) continue;
    const float* __restrict__ bias = a_side ? p.ba : p.bb;
    float* __restrict__ y = a_side ? p.ya : p.yb;
    float bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[i] = (bias && c0 + i < cout) ? bias[c0 + i] : 0.f;
    const bool vec = (cout & 3) == 0 && (reinterpret_cast<size_t>(y) & 15) == 0;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
      const int m = row0 + 32 * g + frow;
      if (m >= M) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[g][4 * q + i];
        v[i] += bv[i];
        if (p.act == HD_ACT_RELU) v[i] = fmaxf(v[i], 0.f);
      }
      float* dst = y + (size_t)m * cout + c0;
      if (vec) {
        const f32x4 o = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(dst) = o;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c0 + i < cout) dst[i] = v[i];
      }
    }
  }
}

int pad4(int c) { return (c + 3) & ~3; }

// ------------------------------------------------------------------ thin-K data-gradient pair
struct ThinDgP {
  const void* ga;
  const void* gb;
  const f16* wa;
  const f16* wb;
  const f16* mask;
  f16* dx;
  long long sa, sb;
  int M, hw, C, Ka, Kb, Kap, Kbp, gf16;
};
struct ThinDgTab {
  ThinDgP p[HD_THIN_MULTI_MAX];
  int first[HD_THIN_MULTI_MAX + 1];
  int n;
  int G;                // 32-pixel groups per wave
};

// the 8 k of this lane's half (k = 8 fh ..) of GEMM row m, rounded as hd_pad_cast_f32_f16 rounds them, zero past K and past M
__device__ __forceinline__ f16x8 thin_grad_frag(const void* g, int gf16, int m, bool ok, int hw, long long stride, int Kr, int Kp, int fh) {
  f16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (f16)0.f;
  if (!ok || 8 * fh >= Kp) return f;
  if (gf16) return ld8g(reinterpret_cast<const f16*>(g) + (size_t)m * Kp + 8 * fh);
  const int n = m / hw, r = m - n * hw;
  const float* src = reinterpret_cast<const float*>(g) + (size_t)n * stride + (size_t)r * Kr;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * fh + j;
    if (k < Kr) f[j] = (f16)src[k];
  }
  return f;
}

template <int NJ>
struct ThinVec;
template <>
struct ThinVec<4> {
  typedef f16x4 T;
  static __device__ __forceinline__ f16 at(const T& v, int j) { return v[j]; }
  static __device__ __forceinline__ void set(T& v, int j, f16 x) { v[j] = x; }
};
template <>
struct ThinVec<1> {
  typedef f16 T;
  static __device__ __forceinline__ f16 at(const T& v, int) { return v; }
  static __device__ __forceinline__ void set(T& v, int, f16 x) { v = x; }
};

// NJ: 32-channel MFMA blocks per pass -- 4 where C % 128 == 0 (8-byte accesses), 1 for any C % 32 == 0 (2-byte accesses: small shapes only)
template <int NJ>
__global__ __launch_bounds__(64) void thin_dgrad_kernel(ThinDgTab t) {
  typedef typename ThinVec<NJ>::T V;
  int pi = 0;
  for (int i = 1; i < t.n; ++i)
    if ((int)blockIdx.x >= t.first[i]) pi = i;
  const ThinDgP p = t.p[pi];
  const int lane = threadIdx.x, c = lane & 31, fh = lane >> 5;
  const int npass = p.C / (32 * NJ);
  const int unit = (int)blockIdx.x - t.first[pi];
  const int pgc = unit / npass, pass = unit - pgc * npass;      // neighbouring waves write neighbouring channel runs of the same pixels
  const int cbase = pass * (32 * NJ) + NJ * c;                   // this lane's NJ consecutive channels
  const int M = p.M, C = p.C;

  f16x8 wfa[NJ], wfb[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
#pragma unroll
    for (int k = 0; k < 8; ++k) wfa[j][k] = wfb[j][k] = (f16)0.f;
    if (8 * fh < p.Kap) wfa[j] = ld8g(p.wa + (size_t)(cbase + j) * p.Kap + 8 * fh);
    if (8 * fh < p.Kbp) wfb[j] = ld8g(p.wb + (size_t)(cbase + j) * p.Kbp + 8 * fh);
  }
  const bool masked = p.mask != nullptr;

  for (int gi = 0; gi < t.G; ++gi) {
    const int m0 = (pgc * t.G + gi) * 32;
    if (m0 >= M) break;
    // mask rows first: they are the long loads
    V mv[16];
    if (masked) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        if (m < M) mv[r] = *reinterpret_cast<const V*>(p.mask + (size_t)m * C + cbase);
      }
    }
    const int mr = m0 + c;
    const f16x8 fa = thin_grad_frag(p.ga, p.gf16, mr, mr < M, p.hw, p.sa, p.Ka, p.Kap, fh);
    const f16x8 fb = thin_grad_frag(p.gb, p.gf16, mr, mr < M, p.hw, p.sb, p.Kb, p.Kbp, fh);
    f32x16 zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
    // the first product leaves rounded to f16 (what the first of the two launches stored)
    f16 ra[NJ][16];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const f32x16 a = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, wfa[j], zero, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) ra[j][r] = (f16)a[r];
    }
    f32x16 accb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) accb[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb, wfb[j], zero, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      if (m >= M) continue;
      V o;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float v = accb[j][r];
        v += (float)ra[j][r];                                   // the residual joins in fp32 (conv_epilogue.h's order: res, bias, mask)
        if (masked) v = ((float)ThinVec<NJ>::at(mv[r], j) > 0.f) ? v : 0.f;
        ThinVec<NJ>::set(o, j, (f16)v);
      }
      *reinterpret_cast<V*>(p.dx + (size_t)m * C + cbase) = o;
    }
  }
}

}  // namespace

// Is this hd_conv2d problem a thin-N forward GEMM?  (1x1 / stride 1 / pad 0 over the stored tensor, nothing fused but bias and ReLU, at
// most 16 output channels, fp32 output in [M][Cout] order: NHWC, or NCHW over 1 x 1 maps)
bool hd_thin_fwd_eligible(const ConvP& p) {
  const bool rows = p.out_mode == HD_OUT_NHWC_F32 || (p.out_mode == HD_OUT_NCHW_F32 && p.Ho * p.Wo == 1);
  return p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && p.in_dil == 1 && !p.x2 && !p.up1 && !p.stats && !p.res && !p.mask &&
         !p.in_scale && !p.pool2 && !p.bs_y && rows && p.Cout <= 16 && (p.act == HD_ACT_NONE || p.act == HD_ACT_RELU) &&
         p.Hin == p.Hsrc && p.Win == p.Wsrc && p.Ho == p.Hin && p.Wo == p.Win;
}

// 32-row groups per wave: two once that still leaves every CU eight waves
int hd_thin_fwd_rg(int64_t rows) { return (rows + 31) / 32 >= 4096 ? 2 : 1; }

// n <= HD_CONV_MULTI_MAX eligible problems in one grid; members that share x, M, K and the activation are paired into one MFMA operand
// where their padded channel counts fit 32 rows (`[cls] * nl + [box] * nl` becomes nl paired problems)
void hd_thin_fwd_launch(const ConvP* ps, int n, hipStream_t s) {
  ThinFwdTab t;
  bool used[HD_CONV_MULTI_MAX] = {};
  int64_t rows = 0;
  t.n = 0;
  for (int i = 0; i < n; ++i) {
    if (used[i]) continue;
    const ConvP& a = ps[i];
    ThinFwdP& q = t.p[t.n++];
    q.x = a.x; q.wa = a.w; q.ba = a.bias; q.ya = (float*)a.y;
    q.wb = nullptr; q.bb = nullptr; q.yb = nullptr;
    q.M = a.M; q.K = a.Ktot; q.ca = a.Cout; q.cap = pad4(a.Cout); q.cb = 0; q.act = a.act;
    for (int j = i + 1; j < n; ++j) {
      const ConvP& b = ps[j];
      if (used[j] || b.x != a.x || b.M != a.M || b.Ktot != a.Ktot || b.act != a.act || q.cap + pad4(b.Cout) > 32) continue;
      q.wb = b.w; q.bb = b.bias; q.yb = (float*)b.y; q.cb = b.Cout;
      used[j] = true;
      break;
    }
    rows += a.M;
  }
  const int rg = hd_thin_fwd_rg(rows);
  int total = 0;
  for (int i = 0; i < t.n; ++i) {
    t.first[i] = total;
    total += hd_cdiv(t.p[i].M, 32 * rg);
  }
  t.first[t.n] = total;
  if (rg == 2) hipLaunchKernelGGL((thin_fwd_kernel<2, 8>), dim3(total), dim3(64), 0, s, t);
  else hipLaunchKernelGGL((thin_fwd_kernel<1, 16>), dim3(total), dim3(64), 0, s, t);
}

static int thin_dgrad_fill(const hd_thin_dgrad_args* a, ThinDgP& q) {
  HD_CHECK_ARG(a && a->ga && a->gb && a->wda && a->wdb && a->dx, "hd_thin_dgrad_pair: null pointer");
  HD_CHECK_ARG(a->n > 0 && a->hw > 0 && (int64_t)a->n * a->hw < (1ll << 31), "hd_thin_dgrad_pair: bad extent");
  HD_CHECK_ARG(a->C > 0 && a->C % 32 == 0, "hd_thin_dgrad_pair: C must be a multiple of 32 (C=%d)", a->C);
  HD_CHECK_ARG((a->Ka_p == 8 || a->Ka_p == 16) && (a->Kb_p == 8 || a->Kb_p == 16) && a->Ka > 0 && a->Ka <= a->Ka_p && a->Kb > 0 && a->Kb <= a->Kb_p,
               "hd_thin_dgrad_pair: Ka_p, Kb_p in {8, 16}, 0 < Ka <= Ka_p, 0 < Kb <= Kb_p");
  HD_CHECK_ARG(a->g_f16 || (a->stride_a >= (int64_t)a->hw * a->Ka && a->stride_b >= (int64_t)a->hw * a->Kb), "hd_thin_dgrad_pair: image stride below hw * K");
  q.ga = a->ga; q.gb = a->gb; q.wa = (const f16*)a->wda; q.wb = (const f16*)a->wdb; q.mask = (const f16*)a->mask; q.dx = (f16*)a->dx;
  q.sa = a->stride_a; q.sb = a->stride_b;
  q.M = a->n * a->hw; q.hw = a->hw; q.C = a->C; q.Ka = a->Ka; q.Kb = a->Kb; q.Kap = a->Ka_p; q.Kbp = a->Kb_p; q.gf16 = a->g_f16 ? 1 : 0;
  return HD_OK;
}

extern "C" int hd_thin_dgrad_pair_multi(const hd_thin_dgrad_args* args, int n, void* stream) {
  HD_CHECK_ARG(args && n >= 1 && n <= HD_THIN_MULTI_MAX, "hd_thin_dgrad_pair_multi: 1 .. %d problems", HD_THIN_MULTI_MAX);
  ThinDgTab t;
  bool wide = true;
  int64_t units = 0;
  for (int i = 0; i < n; ++i) {
    int rc = thin_dgrad_fill(&args[i], t.p[i]);
    if (rc) return rc;
    wide = wide && (t.p[i].C % 128) == 0;
  }
  const int nj = wide ? 4 : 1;
  for (int i = 0; i < n; ++i) units += (int64_t)hd_cdiv(t.p[i].M, 32) * (t.p[i].C / (32 * nj));
  t.n = n;
  t.G = units >= 2048 ? 2 : 1;      // the weights of a pass stay in registers over G pixel groups once the grid is several waves per CU anyway
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    t.first[i] = (int)total;
    total += (int64_t)hd_cdiv(t.p[i].M, 32 * t.G) * (t.p[i].C / (32 * nj));
  }
  HD_CHECK_ARG(total < (1ll << 31), "hd_thin_dgrad_pair_multi: grid too large");
  t.first[n] = (int)total;
  if (wide) hipLaunchKernelGGL((thin_dgrad_kernel<4>), dim3((unsigned)total), dim3(64), 0, (hipStream_t)stream, t);
  else hipLaunchKernelGGL((thin_dgrad_kernel<1>), dim3((unsigned)total), dim3(64), 0, (hipStream_t)stream, t);
  HD_CHECK_LAUNCH();
  return HD_OK;
}

extern "C" int hd_thin_dgrad_pair(const hd_thin_dgrad_args* a, void* stream) { return hd_thin_dgrad_pair_multi(a, 1, stream); }
