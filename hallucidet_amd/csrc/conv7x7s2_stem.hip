// 7x7 / stride 2 / pad 3 convolution, 8 (3 real) -> 64 channels, with the WEIGHTS RESIDENT IN REGISTERS (gfx950): the ResNet stem of
// the hallucination network (src/segmentation_models/encoders/resnet.py:47-52 via torchvision ResNet.conv1 [EXT]; 8 x 512 x 640 with
// BatchNorm partial sums) and of the frozen detector (24 x 300 x 300, folded FrozenBN bias + ReLU).  In the implicit-GEMM family these two
// launches gather a 392-deep K from 16-byte pixels tap by tap (per-lane tap recomputation, 72 and 55 us against a 16 us HBM floor).  Here
// the design of conv_wreg.h; this kernel's own within it:
//   * the 64 x 392 weight matrix is 2 x 25 fragments = 200 AGPRs per lane (none in VGPRs), loaded once per block straight from memory
//     (a lane's 8 K values are one tap's 8 channels: 16 contiguous bytes of a weight row);
//   * the (2*8 + 5) x (2*16 + 5) input patch (777 pixels of 16 bytes: 13 one-KiB DMA pieces, no swizzle) -- stride 2: patch origin -3,
//     two input pixels per output pixel; a K step is two taps, its B fragment one 16-byte read per lane at (2 oy + kh, 2 ox + kw);
//   * the residual / mask operands are requested AFTER the K loop (the 64 -> 64 kernel requests them before it, with a measured reason;
//     no caller gives this kernel either, so nothing was measured here: left as it is).
// K order: tap-major, 8 channels per tap (tap 49 is a zero row) -- the order of the weight layout [64][7*7*8].
#include "conv_wreg.h"

namespace {

constexpr int PH = 2 * TH + 5, PW = 2 * TW + 5;      // 21 x 37 input pixels
constexpr int NPIX = PH * PW;                        // 777
constexpr int NPIECE = (NPIX + 63) / 64;             // 13
constexpr int PPW = (NPIECE + 3) / 4;                // pieces per wave (4; three waves issue 3)
constexpr int STAGE_BYTES = 4 * PPW * 1024;          // 16 KiB
constexpr int KSTEPS = 25, NTAP = 49, KROW = NTAP * 8;
constexpr int RED_OFF = 2 * STAGE_BYTES;             // statistics transpose [4 waves][64][65] floats
constexpr int BIAS_OFF = RED_OFF + 4 * 64 * 65 * 4;  // the bias vector (EPI & 2): read per tile from LDS, not from memory
constexpr int LDS_BYTES = BIAS_OFF + 64 * 4;

// byte offset of tap t inside the patch, relative to the lane's pixel (2 oy, 2 ox); the zero tap re-reads the last real one
__host__ __device__ constexpr int tap_off(int t) { return t < NTAP ? ((t / 7) * PW + (t % 7)) * 16 : ((6 * PW) + 6) * 16; }

// EPI: conv_wreg.h; STATS: BatchNorm partial sums (sum y, sum y^2 of the fp16-rounded output, one row per block)
template <bool STATS, int EPI>
__global__ __launch_bounds__(256) void conv7x7s2_stem_kernel(ConvP p, int tiles_total) {
  __shared__ __attribute__((aligned(1024))) char lds[LDS_BYTES];
  HD_WREG_BLOCK(p, tiles_total);
  const int H = p.Hin, W = p.Win;

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(p.x), 0, p.xbytes, 0x00020000);

  // ---- patch fill tables: piece k of this wave is global piece k * 4 + wave; its lane fetches patch pixel (k * 4 + wave) * 64 + lane
  int rel[PPW], pyx[PPW];
#pragma unroll
  for (int k = 0; k < PPW; ++k) {
    const int pp = (k * 4 + wave) * 64 + lane;
    const int py = pp / PW, px = pp - py * PW;
    rel[k] = ((py - 3) * W + (px - 3)) * 16;
    pyx[k] = wreg_patch_entry(pp, py, px, NPIX);
  }
  auto issue_patch = [&](int n, int ty, int tx, int stage, int k) {
    if (k * 4 + wave >= NPIECE) return;                            // uniform per wave
    const int base = ((n * H + ty * (2 * TH)) * W + tx * (2 * TW)) * 16;
    const bool ok = HD_WREG_PATCH_INSIDE(pyx[k], ty, tx, -3, 2, H, W);
    dma16(rx, lds + stage * STAGE_BYTES + (k * 4 + wave) * 1024, ok ? (unsigned)(base + rel[k]) : OOBB);
  };

  int cn = 0, cty = 0, ctx = 0;
  if (t_begin < t_end) {
    tile_pos(t_begin, cn, cty, ctx);
#pragma unroll
    for (int k = 0; k < PPW; ++k) issue_patch(cn, cty, ctx, 0, k);
  }
  // ---- weights: row 32 b + pl, K step s, half h = tap 2 s + h, all 8 channels (16 contiguous bytes); the 50th tap is a zero row
  f16x8 wr[2][KSTEPS];
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int t = 2 * s + h;
      f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (t < NTAP) v = *reinterpret_cast<const f16x8*>(p.w + (size_t)(32 * b + pl) * KROW + t * 8);
      wr[b][s] = v;
    }

  // ---- B fragments: this lane's output pixel (two tile rows per wave) -> patch pixel (2 oy, 2 ox)
  const int y0l = wreg_y0l(wave, lane), x0l = wreg_x0l(lane);
  const int bbase = ((2 * y0l) * PW + 2 * x0l) * 16;

  float s1[2][16], s2[2][16];
  if (STATS) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) s1[b][r] = s2[b][r] = 0.f;
  }
  const f16* __restrict__ resp = p.res;
  const f16* __restrict__ maskp = p.mask;
  f16* __restrict__ yp = reinterpret_cast<f16*>(p.y);
  if (EPI & 2) {
    if (tid < 64) reinterpret_cast<float*>(lds + BIAS_OFF)[tid] = p.bias[tid];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (ordered against the readers by the tile loop's first barrier)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  for (int t = t_begin; t < t_end; ++t) {
    const int stage = (t - t_begin) & 1;
    __builtin_amdgcn_s_barrier();          // every wave has retired its pieces of tile t and is done reading the other stage
    const bool more = t + 1 < t_end;
    int nn = 0, nty = 0, ntx = 0;
    if (more) tile_pos(t + 1, nn, nty, ntx);
    const char* sb = lds + stage * STAGE_BYTES + bbase;
    f32x16 acc0, acc1;
    f16x8 bf[RING];
#define HD_STEM_B(S) (*reinterpret_cast<const f16x8*>(sb + (h ? tap_off(2 * (S) + 1) : tap_off(2 * (S)))))
#pragma unroll
    for (int s = 0; s < RING; ++s) bf[s] = HD_STEM_B(s);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const f16x8 cur = bf[s % RING];
      if (s == 0) {
        HD_WREG_MFMA0_A(acc0, wr[0][s], cur);
        HD_WREG_MFMA0_A(acc1, wr[1][s], cur);
      } else {
        HD_WREG_MFMA_A(acc0, wr[0][s], cur);
        HD_WREG_MFMA_A(acc1, wr[1][s], cur);
      }
      if (s + RING < KSTEPS) bf[s % RING] = HD_STEM_B(s + RING);
      if (s % 6 == 1 && more) issue_patch(nn, nty, ntx, stage ^ 1, s / 6);      // s = 1, 7, 13, 19: the four pieces of the next patch
    }
#undef HD_STEM_B
    HD_WREG_DRAIN(acc0, acc1);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- epilogue in registers: acc{b}[4g + i] = channel 32b + 8g + 4h + i of this lane's pixel
    const wreg_pixel px = wreg_out_pixel<64>(p, y0l, x0l, cn, cty, ctx);
    const bool okp = px.ok;
    f16x4 rv[8], mv[8];
    f32x4 bv[8];
    if (EPI & 1) HD_WREG_LOAD_QUADS(rv, resp, px, h);          // (after the K loop: see the header comment)
    if (EPI & 4) HD_WREG_LOAD_QUADS(mv, maskp, px, h);
    if (EPI & 2) {
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = *reinterpret_cast<const f32x4*>(lds + BIAS_OFF + (8 * j + 4 * h) * 4);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int gp = 0; gp < 4; gp += 2) {
        unsigned pk[2][2];
#pragma unroll
        for (int gg = 0; gg < 2; ++gg) {
          const int g = gp + gg, j = 4 * b + g;
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = b ? acc1[4 * g + i] : acc0[4 * g + i];
          HD_WREG_EPI_OPERANDS(EPI, v, rv[j], bv[j], mv[j]);
          if (STATS) HD_WREG_STATS_ADD(v, okp, s1[b], s2[b], g);
          if (EPI & 8) wreg_epi_relu(v);
          wreg_pack(v, pk[gg]);
        }
        const u32x4 o = wreg_exchange(pk);
        if (okp) *reinterpret_cast<u32x4*>(yp + px.eoff + 32 * b + 8 * (gp + h)) = o;
      }
    cn = nn; cty = nty; ctx = ntx;
    __builtin_amdgcn_sched_barrier(0);
  }

  if (STATS) HD_WREG_FOLD_STATS(64, false, p, lds, RED_OFF, 0, &s1[0][0], &s2[0][0], (const float*)nullptr);
}

}  // namespace

// 7x7 / s2 / p3, one 8-channel source, 64 output channels, NHWC f16 out.  (Nothing here may depend on p.stats.)
bool hd_conv_stem_eligible(const ConvP& p) {
  if (p.KH != 7 || p.KW != 7 || p.stride != 2 || p.pad != 3 || p.in_dil != 1 || p.up1) return false;
  if (p.C1 != 8 || p.C2 != 0 || p.x2 || p.Cout != 64 || p.out_mode != HD_OUT_NHWC_F16 || p.in_scale || p.bs_y) return false;
  if (p.Hsrc != p.Hin || p.Wsrc != p.Win || p.Ho != (p.Hin + 6 - 7) / 2 + 1 || p.Wo != (p.Win + 6 - 7) / 2 + 1) return false;
  if (p.act != HD_ACT_NONE && p.act != HD_ACT_RELU) return false;
  if (p.xbytes & 0xC0000000u) return false;
  if ((int64_t)p.N * p.Ho * p.Wo * 64 >= (int64_t)1 << 31) return false;
  return true;
}

int hd_conv_stem_rows(const ConvP& p) { return hd_wreg_rows(p); }

void hd_conv_launch_stem(ConvP& p, hipStream_t s) { HD_WREG_LAUNCH_EPI(conv7x7s2_stem_kernel, false, true, p, s) }
