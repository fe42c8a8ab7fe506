// 3x3 / stride 1 / pad 1 convolution over cat([nearest_2x(a), skip]) with 64 + 64 input and 32 output channels, WEIGHTS RESIDENT IN
// REGISTERS (gfx950): decoder block 3's first convolution of the hallucination network at 256 x 320
// (src/segmentation_models/decoders/unet/decoder.py:37-46: F.interpolate(x, 2) -> torch.cat -> Conv2dReLU; 48 GFLOP, 117 us in the 4-wave
// implicit-GEMM family whose 32-wide N tile re-gathers the 1 152-deep K for every 128 pixels).  The 32 x 1 152 weight matrix is 72 KiB --
// the size conv3x3_c64.hip keeps in registers -- so the same design (conv_wreg.h) applies, with the upsample + concat folded into the
// patch DMA; this kernel's own within it:
//   * a wave owns 32 pixels x all 32 channels: 72 A fragments per lane (one cout block x 72 K steps; 64 in AGPRs, 8 in VGPRs), loaded
//     once per block straight from memory;
//   * TWO patches of 128-byte pixels per tile, each laid out and swizzled exactly as the 64-channel kernel's: region A holds
//     a[(y >> 1), (x >> 1)] (the nearest-2x upsample is a halved source coordinate), region B holds skip[y, x]; an LDS-DMA instruction
//     takes one buffer resource, so the two sources never share a 1-KiB piece; 2 x 23 pieces per tile;
//   * a K step is (tap, 16-channel block): blocks 0..3 read region A, 4..7 region B; even and odd K steps accumulate into two independent
//     chains that are added in the epilogue; no epilogue operands;
//   * the sums are those of 32 channels: the fold's `lane < 32` guards and its extra barrier.
// K order: tap-major, the 64 upsampled then the 64 skip channels, 16 at a time -- the order of the implicit-GEMM kernels.
#include "conv_wreg.h"

namespace {

constexpr int PH = TH + 2, PW = TW + 2;
constexpr int NPIX = PH * PW;                        // 180 patch pixels of 128 bytes per region
constexpr int PIECES = 6;                            // 1-KiB DMA pieces per wave per region (4 x 6 = 24 >= 22.5)
constexpr int REGION_BYTES = 4 * PIECES * 1024;      // 24 KiB
constexpr int STAGE_BYTES = 2 * REGION_BYTES;        // 48 KiB
constexpr int KSTEPS = 72, KROW = 1152;
constexpr int LDS_BYTES = 2 * STAGE_BYTES;           // 96 KiB

constexpr int NA = 64;         // K steps whose weight fragment lives in AGPRs (64 x 4 = 256 registers)

template <bool STATS>
__global__ __launch_bounds__(256) void conv3x3_cat128to32_kernel(ConvP p, int tiles_total) {
  __shared__ __attribute__((aligned(1024))) char lds[LDS_BYTES];
  HD_WREG_BLOCK(p, tiles_total);
  const int H = p.Hin, W = p.Win, Hs = p.Hsrc, Ws = p.Wsrc;

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(p.x), 0, p.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(p.x2), 0, p.x2bytes, 0x00020000);

  // ---- patch fill tables (both regions): unit u = (k*4 + wave)*64 + lane is 16-byte slot (u & 7) of patch pixel u >> 3
  int relu_[PIECES], rels_[PIECES], pyx[PIECES];
#pragma unroll
  for (int k = 0; k < PIECES; ++k) {
    const int u = (k * 4 + wave) * 64 + lane;
    const int pp = u >> 3, slot = u & 7;
    const int py = (pp * 3641) >> 16, px = pp - py * PW;          // pp / 18 (exact for pp < 2 000)
    const int cg = slot ^ ((px >> 1) & 7);
    relu_[k] = (((py - 1) >> 1) * Ws + ((px - 1) >> 1)) * 128 + cg * 16;     // upsampled source: halved coordinates (floor, also for -1)
    rels_[k] = ((py - 1) * W + (px - 1)) * 128 + cg * 16;
    pyx[k] = wreg_patch_entry(pp, py, px, NPIX);
  }
  // piece k (0 .. 2*PIECES-1) of the next patch: k < PIECES region A (upsampled source), else region B (skip source)
  auto issue_patch = [&](int n, int ty, int tx, int stage, int k) {
    const int kk = k < PIECES ? k : k - PIECES;
    const bool ok = HD_WREG_PATCH_INSIDE(pyx[kk], ty, tx, -1, 1, H, W);
    if (k < PIECES) {
      const int base = ((n * Hs + ty * (TH / 2)) * Ws + tx * (TW / 2)) * 128;
      dma16(rx, lds + stage * STAGE_BYTES + (kk * 4 + wave) * 1024, ok ? (unsigned)(base + relu_[kk]) : OOBB);
    } else {
      const int base = ((n * H + ty * TH) * W + tx * TW) * 128;
      dma16(rx2, lds + stage * STAGE_BYTES + REGION_BYTES + (kk * 4 + wave) * 1024, ok ? (unsigned)(base + rels_[kk]) : OOBB);
    }
  };

  int cn = 0, cty = 0, ctx = 0;
  if (t_begin < t_end) {
    tile_pos(t_begin, cn, cty, ctx);
#pragma unroll
    for (int k = 0; k < 2 * PIECES; ++k) issue_patch(cn, cty, ctx, 0, k);
  }
  // ---- weights: row pl (cout), K step s, half h: K values 16 s + 8 h .. + 7 = 16 contiguous bytes of the row
  f16x8 wr[KSTEPS];
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s) wr[s] = *reinterpret_cast<const f16x8*>(p.w + (size_t)pl * KROW + s * 16 + h * 8);

  // ---- B fragment addresses: this lane's pixel (two tile rows per wave) at tap (kh, kw), 16-channel group c of a region, half h
  const int y0l = wreg_y0l(wave, lane), x0l = wreg_x0l(lane);
  int ab[3][4];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const int xk = x0l + kw;
#pragma unroll
    for (int c = 0; c < 4; ++c) ab[kw][c] = (y0l * PW + xk) * 128 + (((2 * c + h) ^ ((xk >> 1) & 7)) & 7) * 16;
  }

  float s1[16], s2[16];
  if (STATS) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s1[r] = s2[r] = 0.f;
  }
  f16* __restrict__ yp = reinterpret_cast<f16*>(p.y);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  for (int t = t_begin; t < t_end; ++t) {
    const int stage = (t - t_begin) & 1;
    __builtin_amdgcn_s_barrier();          // every wave has retired its pieces of tile t and is done reading the other stage
    const bool more = t + 1 < t_end;
    int nn = 0, nty = 0, ntx = 0;
    if (more) tile_pos(t + 1, nn, nty, ntx);
    const char* sb = lds + stage * STAGE_BYTES;
    f32x16 acc0, acc1;
    f16x8 bf[RING];
    // K step s: tap s >> 3 = (kh, kw); 16-channel block s & 7: region (s & 7) >> 2, group (s & 3)
#define HD_CAT_B(S) (*reinterpret_cast<const f16x8*>(sb + (((S) & 7) >> 2) * REGION_BYTES + ab[((S) >> 3) % 3][(S) & 3] + ((S) / 24) * (PW * 128)))
#pragma unroll
    for (int s = 0; s < RING; ++s) bf[s] = HD_CAT_B(s);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const f16x8 cur = bf[s % RING];
      if (s == 0) HD_WREG_MFMA0_A(acc0, wr[s], cur);
      else if (s == 1) HD_WREG_MFMA0_A(acc1, wr[s], cur);
      else if (s < NA) {
        if (s & 1) HD_WREG_MFMA_A(acc1, wr[s], cur);
        else HD_WREG_MFMA_A(acc0, wr[s], cur);
      } else {
        if (s & 1) HD_WREG_MFMA_V(acc1, wr[s], cur);
        else HD_WREG_MFMA_V(acc0, wr[s], cur);
      }
      if (s + RING < KSTEPS) bf[s % RING] = HD_CAT_B(s + RING);
      // the next tile's two patches: one piece every six K steps (12 pieces over 72 steps)
      if (s % 6 == 1 && more) issue_patch(nn, nty, ntx, stage ^ 1, s / 6);
    }
#undef HD_CAT_B
    HD_WREG_DRAIN(acc0, acc1);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- epilogue in registers: (acc0 + acc1)[4g + i] = channel 8g + 4h + i of this lane's pixel
    const wreg_pixel px = wreg_out_pixel<32>(p, y0l, x0l, cn, cty, ctx);
    const bool okp = px.ok;
#pragma unroll
    for (int gp = 0; gp < 4; gp += 2) {
      unsigned pk[2][2];
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const int g = gp + gg;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = acc0[4 * g + i] + acc1[4 * g + i];
        if (STATS) HD_WREG_STATS_ADD(v, okp, s1, s2, g);
        wreg_pack(v, pk[gg]);
      }
      const u32x4 o = wreg_exchange(pk);
      if (okp) *reinterpret_cast<u32x4*>(yp + px.eoff + 8 * (gp + h)) = o;
    }
    cn = nn; cty = nty; ctx = ntx;
    __builtin_amdgcn_sched_barrier(0);
  }

  if (STATS) HD_WREG_FOLD_STATS(32, false, p, lds, 0, 4 * 32 * 65 * 4, s1, s2, (const float*)nullptr);
}

}  // namespace

// 3x3 / s1 / p1 over cat([nearest_2x(x), x2]) with 64 + 64 input channels, 32 output channels, plain NHWC f16 output (+ BN partial sums).
// (Nothing here may depend on p.stats.)
bool hd_conv_cat128to32_eligible(const ConvP& p) {
  if (p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1 || p.in_dil != 1 || !p.up1 || !p.x2) return false;
  if (p.C1 != 64 || p.C2 != 64 || p.Cout != 32 || p.out_mode != HD_OUT_NHWC_F16) return false;
  if (p.Ho != p.Hin || p.Wo != p.Win || p.Hin != 2 * p.Hsrc || p.Win != 2 * p.Wsrc || p.in_scale || p.bs_y) return false;
  if (p.act != HD_ACT_NONE || p.bias || p.res || p.mask) return false;
  if ((p.xbytes | p.x2bytes) & 0xC0000000u) return false;
  return true;
}

int hd_conv_cat128to32_rows(const ConvP& p) { return hd_wreg_rows(p); }

void hd_conv_launch_cat128to32(ConvP& p, hipStream_t s) {
  const dim3 grid(hd_wreg_rows(p));
  if (p.stats) hipLaunchKernelGGL((conv3x3_cat128to32_kernel<true>), grid, dim3(256), 0, s, p, hd_wreg_tiles(p));
  else hipLaunchKernelGGL((conv3x3_cat128to32_kernel<false>), grid, dim3(256), 0, s, p, hd_wreg_tiles(p));
}
