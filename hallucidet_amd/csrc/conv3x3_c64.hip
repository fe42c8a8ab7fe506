// 3x3 / stride 1 / pad 1 convolution, 64 -> 64 channels, with the WEIGHTS RESIDENT IN REGISTERS (gfx950).
//
// The layers: ResNet-34 layer1 of the hallucination network at 128x160 (six forward convolutions with BatchNorm partial sums, their data
// gradients with the residual add; reference src/segmentation_models/encoders/resnet.py:47-65 via torchvision BasicBlock [EXT]) and the
// 3x3 of the detector's layer1 bottlenecks at 75x75 (bias + ReLU; data gradient with the ReLU mask).  M is huge (163 840 pixels), N = 64,
// K = 576: in the implicit-GEMM family a 128 x 64 tile lives for nine K steps, and its set-up + LDS epilogue cost more than its MFMAs
// (27-30 us per launch against a 5 us floor).  Two earlier attempts kept the weight matrix in LDS (49 us: 1.5 KiB of fragment reads per
// MFMA, LDS-bound) -- here the 64 x 576 matrix is the MFMA *A* operand and never leaves the register file.
// This is the first kernel of the design that conv_wreg.h describes; its own within it:
//   * a wave owns 32 pixels x all 64 output channels: 2 x 36 A fragments = 288 registers of weights (64 fragments in AGPRs, 8 in
//     VGPRs), loaded once per block through LDS (LDS-DMA of the matrix as it lies in memory, source-side swizzle, 72 conflict-free
//     ds_read_b128) -- the siblings read theirs straight from memory;
//   * per 16-deep K step ONE 1-KiB fragment read (the pixels, B operand) feeds TWO v_mfma_f32_32x32x16_f16: 144 KiB of LDS reads
//     per 2 304 MFMA clocks of a tile (the LDS port would carry 288);
//   * the (8+2) x (16+2) input patch of 128-byte pixels, swizzle slot ^= (x >> 1) & 7 on the source side: conflict-free for all three
//     kw under ds_read_b128's 16-lane groups because the patch pitch (18 pixels) is even, so a pixel's 128-byte row alternates between
//     the two halves of the 256-byte bank row with x;
//   * the residual / ReLU-mask operands are requested BEFORE the K loop (measured, see the tile loop);
//   * STATS 2, 3: the BatchNorm BACKWARD sums of a data gradient, and the HD_TRACE stamps.
// K order is tap-major, 16 channels at a time -- the order the implicit-GEMM kernels accumulate in.
#include "conv_wreg.h"

namespace {

constexpr int PH = TH + 2, PW = TW + 2;
constexpr int NPIX = PH * PW;                    // 180 patch pixels of 128 bytes
constexpr int PIECES = 6;                        // 1-KiB DMA pieces per wave per patch (4 x 6 = 24 >= 22.5)
constexpr int STAGE_BYTES = 4 * PIECES * 1024;   // 24 KiB
constexpr int KTOT = 576, KSTEPS = 36;
constexpr int W_OFF = 2 * STAGE_BYTES;           // weight staging (72 KiB), later the statistics transpose
constexpr int W_BYTES = 64 * KTOT * 2;
constexpr int LDS_BYTES = W_OFF + W_BYTES;       // 120 KiB: one block per CU
constexpr int CF_OFF = W_OFF + 4 * 64 * 65 * 4;  // per-channel coefficients of the bs_* modes: behind the statistics transpose, inside the weight staging
constexpr int BIAS_OFF = CF_OFF + 4 * 64 * 4;    // the bias vector (EPI & 2): read per tile from LDS, not from memory
static_assert(BIAS_OFF + 64 * 4 <= LDS_BYTES, "coefficient table and bias fit");

constexpr int NA = 32;         // K steps whose two weight fragments live in AGPRs (2 x 32 x 4 = 256 registers)

// EPI: conv_wreg.h
// STATS: 0 none | 1 BatchNorm forward sums (sum y, sum y^2) | 2, 3 hd_conv_args.bs_*: the output is the gradient dz of a BatchNorm unit and
// its BACKWARD sums (sum dz*m, sum dz*m*xhat) leave through the same rows -- ReLU mask m recomputed from the unit's y (2) or read from
// its saved activation z (3); per-channel coefficients sit in the dead weight-staging area of LDS
template <int STATS, int EPI>
__global__ __launch_bounds__(256) void conv3x3_c64_kernel(ConvP p, int tiles_total) {
  __shared__ __attribute__((aligned(1024))) char lds[LDS_BYTES];
  HD_TRACE(0, wall_clock64());
  HD_TRACE(1, clock64());
  HD_WREG_BLOCK(p, tiles_total);
#ifdef HD_CONV_TRACE
  long long tr_bar = 0, tr_k = 0, tr_wait = 0, tr_epi = 0, tr_t = 0;
#define TR_MARK(accu) do { long long n_ = clock64(); accu += n_ - tr_t; tr_t = n_; } while (0)
#else
#define TR_MARK(accu) do {} while (0)
#endif

  const int H = p.Hin, W = p.Win;

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(p.x), 0, p.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(p.w), 0, p.wbytes, 0x00020000);

  // ---- patch fill tables: unit u = (k*4 + wave)*64 + lane is 16-byte slot (u & 7) of patch pixel u >> 3
  int rel[PIECES], pyx[PIECES];
#pragma unroll
  for (int k = 0; k < PIECES; ++k) {
    const int u = (k * 4 + wave) * 64 + lane;
    const int pp = u >> 3, slot = u & 7;
    const int py = (pp * 3641) >> 16, px = pp - py * PW;          // pp / 18 (exact for pp < 2 000)
    const int cg = slot ^ ((px >> 1) & 7);
    rel[k] = ((py - 1) * W + (px - 1)) * 128 + cg * 16;
    pyx[k] = wreg_patch_entry(pp, py, px, NPIX);
  }
  auto issue_patch = [&](int n, int ty, int tx, int stage, int k) {
    const int base = ((n * H + ty * TH) * W + tx * TW) * 128;
    const bool ok = HD_WREG_PATCH_INSIDE(pyx[k], ty, tx, -1, 1, H, W);
    dma16(rx, lds + stage * STAGE_BYTES + (k * 4 + wave) * 1024, ok ? (unsigned)(base + rel[k]) : OOBB);
  };

  // ---- prologue: first patch + the weight matrix in flight together
  int cn = 0, cty = 0, ctx = 0;
  if (t_begin < t_end) {
    tile_pos(t_begin, cn, cty, ctx);
#pragma unroll
    for (int k = 0; k < PIECES; ++k) issue_patch(cn, cty, ctx, 0, k);
  }
#pragma unroll
  for (int k = 0; k < 18; ++k) {
    const int u = (k * 4 + wave) * 64 + lane;                    // 16-byte chunk index of the [64][576] matrix
    const int row = (u * 58255) >> 22, j = u - row * 72;          // u / 72 (exact for u < 4 608)
    const int src = (j & ~7) | ((j & 7) ^ ((row >> 1) & 7));
    dma16(rw, lds + W_OFF + (k * 4 + wave) * 1024, (unsigned)(row * (KTOT * 2) + src * 16));
  }
  HD_TRACE(2, clock64());
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  HD_TRACE(3, clock64());
  f16x8 wr[2][KSTEPS];
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int row = 32 * b + pl, q = 2 * s + h;
      const int slot = (q & ~7) | ((q & 7) ^ ((row >> 1) & 7));
      wr[b][s] = *reinterpret_cast<const f16x8*>(lds + W_OFF + row * (KTOT * 2) + slot * 16);
    }

  if (EPI & 2) {
    __syncthreads();                                    // every wave has its weight fragments: the staging area is free
    if (tid < 64) reinterpret_cast<float*>(lds + BIAS_OFF)[tid] = p.bias[tid];
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // (ordered against the readers by the tile loop's first barrier)
  }
  if (STATS >= 2) {
    __syncthreads();                                    // every wave has its weight fragments: the staging area is free
    float* cf = reinterpret_cast<float*>(lds + CF_OFF);  // [mean | invstd | scale | shift][64]
    if (tid < 64) {
      const float mu = p.bs_mean[tid], is = p.bs_invstd[tid];
      const float g = p.bs_gamma ? p.bs_gamma[tid] : 1.f, b = p.bs_beta ? p.bs_beta[tid] : 0.f;
      cf[tid] = mu;
      cf[64 + tid] = is;
      cf[128 + tid] = g * is;
      cf[192 + tid] = b - mu * g * is;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (ordered against the readers by the tile loop's first barrier)
  }

  // ---- B fragment addresses: this lane's pixel (two tile rows per wave) at tap (kh, kw), 16-channel group c, half h
  const int y0l = wreg_y0l(wave, lane), x0l = wreg_x0l(lane);
  int ab[3][4];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const int xk = x0l + kw;
#pragma unroll
    for (int c = 0; c < 4; ++c) ab[kw][c] = (y0l * PW + xk) * 128 + (((2 * c + h) ^ ((xk >> 1) & 7)) & 7) * 16;
  }

  float s1[2][16], s2[2][16];
  if (STATS != 0) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) s1[b][r] = s2[b][r] = 0.f;
  }
  HD_TRACE(4, clock64());
#ifdef HD_CONV_TRACE
  tr_t = clock64();
#endif
  const f16* __restrict__ resp = p.res;
  const f16* __restrict__ maskp = p.mask;
  f16* __restrict__ yp = reinterpret_cast<f16*>(p.y);

  for (int t = t_begin; t < t_end; ++t) {
    const int stage = (t - t_begin) & 1;
    // every wave has retired its pieces of tile t (vmcnt(0) below / in the prologue) and is done reading the other stage
    __builtin_amdgcn_s_barrier();
    TR_MARK(tr_bar);
    const bool more = t + 1 < t_end;
    int nn = 0, nty = 0, ntx = 0;
    if (more) tile_pos(t + 1, nn, nty, ntx);
    const char* sb = lds + stage * STAGE_BYTES;
    // bs_* modes: the unit's y (and z) vectors of this tile are requested BEFORE the K loop -- after it they were an exposed HBM round trip
    // per tile on a kernel that runs one wave per SIMD (the 64-channel data gradients read 31.7 us with the sums against 17.7 without)
    f16x4 byv[8], bzv[8], rv[8], mv[8];
    // (each request computes this lane's pixel for itself, and the epilogue again: computed once up here it changed the sums variants' code)
    if (EPI & 4) {          // the ReLU-mask operand likewise
      const wreg_pixel px = wreg_out_pixel<64>(p, y0l, x0l, cn, cty, ctx);
      HD_WREG_LOAD_QUADS(mv, maskp, px, h);
    }
    if (EPI & 1) {          // the residual operand too (requested after the K loop, where the stem requests its own, it cost the residual variants 7 us per launch)
      const wreg_pixel px = wreg_out_pixel<64>(p, y0l, x0l, cn, cty, ctx);
      HD_WREG_LOAD_QUADS(rv, resp, px, h);
    }
    if (STATS >= 2) {
      const wreg_pixel px = wreg_out_pixel<64>(p, y0l, x0l, cn, cty, ctx);
      HD_WREG_LOAD_QUADS(byv, p.bs_y, px, h);
      if (STATS == 3) HD_WREG_LOAD_QUADS(bzv, p.bs_z, px, h);
    }
    f32x16 acc0, acc1;
    f16x8 bf[RING];
#define HD_C64_B(S) (*reinterpret_cast<const f16x8*>(sb + ab[((S) >> 2) % 3][(S) & 3] + ((S) / 12) * (PW * 128)))
#pragma unroll
    for (int s = 0; s < RING; ++s) bf[s] = HD_C64_B(s);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const f16x8 cur = bf[s % RING];
      if (s == 0) {
        HD_WREG_MFMA0_A(acc0, wr[0][s], cur);
        HD_WREG_MFMA0_A(acc1, wr[1][s], cur);
      } else if (s < NA) {
        HD_WREG_MFMA_A(acc0, wr[0][s], cur);
        HD_WREG_MFMA_A(acc1, wr[1][s], cur);
      } else {
        HD_WREG_MFMA_V(acc0, wr[0][s], cur);
        HD_WREG_MFMA_V(acc1, wr[1][s], cur);
      }
      if (s + RING < KSTEPS) bf[s % RING] = HD_C64_B(s + RING);
      // the next tile's patch: one piece every six K steps (issued back to back a piece cost this wave ~150 clocks, spread out ~70)
      if (s % 6 == 1 && more) issue_patch(nn, nty, ntx, stage ^ 1, s / 6);
    }
#undef HD_C64_B
    HD_WREG_DRAIN(acc0, acc1);
    __builtin_amdgcn_sched_barrier(0);
    TR_MARK(tr_k);
    // the next tile's pieces: the last one was issued five K steps ago, nothing younger than them is outstanding
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TR_MARK(tr_wait);

    // ---- epilogue in registers: acc{b}[4g + i] = channel 32b + 8g + 4h + i of this lane's pixel
    const wreg_pixel px = wreg_out_pixel<64>(p, y0l, x0l, cn, cty, ctx);          // offsets < 2^30 elements (eligibility)
    const bool okp = px.ok;
    f32x4 bv[8];
    if (EPI & 2) {
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = *reinterpret_cast<const f32x4*>(lds + BIAS_OFF + (8 * j + 4 * h) * 4);
    }
    // rv / y / z vectors of the whole tile are requested up front; the packed output of a group pair is exchanged and stored as soon
    // as it exists (a separate store pass would keep all sixteen packed registers alive next to the resident weights)
    // STATS 2: (scale, shift) of this lane's channels for the ReLU mask, re-read per tile through an offset the compiler cannot see
    // through (hoisted out of the tile loop the 64 floats push weight fragments into scratch)
    int tile_zero = 0;
    if (STATS == 2) asm volatile("v_mov_b32 %0, 0" : "=v"(tile_zero));
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int gp = 0; gp < 4; gp += 2) {
        unsigned pk[2][2];                 // groups gp, gp + 1: four channels each as two packed f16 pairs
#pragma unroll
        for (int gg = 0; gg < 2; ++gg) {
          const int g = gp + gg, j = 4 * b + g;
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = b ? acc1[4 * g + i] : acc0[4 * g + i];
          HD_WREG_EPI_OPERANDS(EPI, v, rv[j], bv[j], mv[j]);
          if (STATS == 1) HD_WREG_STATS_ADD(v, okp, s1[b], s2[b], g);
          if (STATS >= 2) {
            // sum dz*m and sum dz*m*y of this lane's channels 8j + 4h .. + 3 on the fp16-rounded dz; sum dz*m*xhat =
            // invstd * (sum dz*m*y - mean * sum dz*m) is formed once per block below (no per-channel mean / invstd in this loop)
            f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = sc;
            if (STATS == 2) {
              const float* cf = reinterpret_cast<const float*>(lds + CF_OFF + tile_zero) + 8 * j + 4 * h;
              sc = *reinterpret_cast<const f32x4*>(cf + 128);
              sh = *reinterpret_cast<const f32x4*>(cf + 192);
            }
            const float keep = okp ? 1.f : 0.f;
            const bool relu = p.bs_relu != 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float gk = (float)(f16)v[i] * keep;
              const float yk = (float)byv[j][i];
              const bool on = STATS == 3 ? ((float)bzv[j][i] > 0.f) : ((float)(f16)hd_bn_affine(yk, sc[i], sh[i]) > 0.f);
              gk = (on || !relu) ? gk : 0.f;
              s1[b][4 * g + i] += gk;
              s2[b][4 * g + i] += gk * yk;
            }
          }
          if (EPI & 8) wreg_epi_relu(v);
          wreg_pack(v, pk[gg]);
        }
        const u32x4 o = wreg_exchange(pk);
        if (okp) *reinterpret_cast<u32x4*>(yp + px.eoff + 32 * b + 8 * (gp + h)) = o;
      }
    cn = nn; cty = nty; ctx = ntx;
    __builtin_amdgcn_sched_barrier(0);
    TR_MARK(tr_epi);
  }
  HD_TRACE(5, clock64());
#ifdef HD_CONV_TRACE
  HD_TRACE(8, (unsigned long long)tr_bar);
  HD_TRACE(9, (unsigned long long)tr_k);
  HD_TRACE(10, (unsigned long long)tr_wait);
  HD_TRACE(11, (unsigned long long)tr_epi);
  HD_TRACE(12, (unsigned long long)(t_end - t_begin));
#endif

  // the sums leave through the dead weight staging (transpose) and patch stages; STATS >= 2: sum dz*m*xhat is formed from sum dz*m*y here
  if (STATS != 0) HD_WREG_FOLD_STATS(64, STATS >= 2, p, lds, W_OFF, 0, &s1[0][0], &s2[0][0], reinterpret_cast<const float*>(lds + CF_OFF));
  HD_TRACE(13, clock64());
  HD_TRACE(6, wall_clock64());
  HD_TRACE(7, hw_ids());
}

}  // namespace

// 3x3 / s1 / p1, one 64-channel source, 64 output channels, NHWC f16 out, same extent in and out, no sigmoid.  (Nothing here may depend
// on p.stats: hd_conv2d_stats_rows asks before the slab exists.)
bool hd_conv_c64_eligible(const ConvP& p) {
  if (p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1 || p.in_dil != 1 || p.up1) return false;
  if (p.C1 != 64 || p.C2 != 0 || p.x2 || p.Cout != 64 || p.out_mode != HD_OUT_NHWC_F16) return false;
  if (p.Ho != p.Hin || p.Wo != p.Win || p.Hsrc != p.Hin || p.Wsrc != p.Win || p.in_scale) return false;
  if (p.act != HD_ACT_NONE && p.act != HD_ACT_RELU) return false;
  if ((p.xbytes | p.wbytes) & 0xC0000000u) return false;      // out-of-range lanes are marked by bit 31 of the offset; element offsets fit 30 bits
  return true;
}

int hd_conv_c64_rows(const ConvP& p) { return hd_wreg_rows(p); }

void hd_conv_launch_c64(ConvP& p, hipStream_t s) {
  if (p.bs_y) {          // BatchNorm backward sums (data gradients: plain or + residual; fill_params excludes bias / mask / act)
    const dim3 grid(hd_wreg_rows(p));
    const int tiles = hd_wreg_tiles(p);
    if (p.bs_z) {
      if (p.res) hipLaunchKernelGGL((conv3x3_c64_kernel<3, 1>), grid, dim3(256), 0, s, p, tiles);
      else hipLaunchKernelGGL((conv3x3_c64_kernel<3, 0>), grid, dim3(256), 0, s, p, tiles);
    } else {
      if (p.res) hipLaunchKernelGGL((conv3x3_c64_kernel<2, 1>), grid, dim3(256), 0, s, p, tiles);
      else hipLaunchKernelGGL((conv3x3_c64_kernel<2, 0>), grid, dim3(256), 0, s, p, tiles);
    }
    return;
  }
  HD_WREG_LAUNCH_EPI(conv3x3_c64_kernel, 0, 1, p, s)
}
