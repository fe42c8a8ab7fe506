// Scaffold of the convolution kernels that keep their WEIGHTS IN REGISTERS (gfx950): conv3x3_c64.hip, conv7x7s2_stem.hip,
// conv3x3_c32to128.hip, conv3x3_cat128to32.hip.  A fifth kernel of this family starts from here.  The design they share:
//   * 4 waves per block, ONE wave per SIMD, one persistent block per CU walking a contiguous run of 8 x 16-pixel output tiles;
//   * a wave owns 32 pixels (two tile rows) x up to 64 output channels at a time;
//   * the weight matrix (72 KiB at most) is the MFMA *A* operand, loaded once per block and pinned in the register file by inline-assembly
//     "a" constraints (up to 64 fragments = all 256 AGPRs, the rest in VGPRs); the pixels are the B operand, one 16-byte LDS read per
//     lane and 16-deep K step through a ring of fragments in flight;
//   * the input patch of the NEXT tile arrives by LDS-DMA during the K loop (two stages, hardware zero-fill for the padding), one 1-KiB
//     piece per wave every six K steps;
//   * C[cout][pixel]: a lane ends up with 4 consecutive output channels of one pixel per accumulator quad -> the epilogue runs in
//     registers (residual / bias / ReLU mask / activation, half exchange, 16-byte stores), no LDS transpose, no barrier;
//   * BatchNorm partial sums accumulate in registers over all tiles of the block and are folded ONCE per block (LDS transpose, fixed
//     order: deterministic); one partial row per block.
// What stays in each kernel's file is its own: LDS layout, weight load, patch byte offsets and swizzle, B-fragment addressing, the
// accumulator pattern of its K loop and the tile loop around it.  Register pressure is at the edge (256 AGPRs of weights + up to 32 VGPR
// fragments) and none of the kernels may use scratch.  The pieces here are forced-inline functions where that left the kernels'
// instruction streams as they were, and macros (said at each) where a function -- a reference to one of the kernel's arrays, a struct
// member -- changed schedules or register allocation: compare the assembly of all four files before turning one into the other.
#pragma once
#include "hd_common.h"
#include "conv_params.h"
#include "hd_lds_dma.h"

// The MFMAs are inline assembly so that the weight fragments can be PINNED in the accumulator file ("a" operands; what does not fit the
// 256 AGPRs stays in VGPRs: _V): left to the register allocator they were spilled to AGPRs and copied back with four v_accvgpr_read per
// MFMA (64 -> 64 kernel: K loop 3 800 clocks per tile without any DMA, 8 000 in the statistics variant; MFMA work: 2 304).
// What the compiler therefore does not see and the code provides: the wait states between the last MFMA of a tile and the first VALU
// read of its accumulators (HD_WREG_DRAIN); an accumulator that is both SrcC and vDst of back-to-back MFMAs needs none.
#define HD_WREG_MFMA0_A(ACC, WF, BF) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(ACC) : "a"(WF), "v"(BF))
#define HD_WREG_MFMA_A(ACC, WF, BF) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(ACC) : "a"(WF), "v"(BF))
#define HD_WREG_MFMA_V(ACC, WF, BF) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(ACC) : "v"(WF), "v"(BF))
#define HD_WREG_DRAIN(A0, A1) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(A0), "+v"(A1))

namespace {

constexpr int TH = 8, TW = 16;      // output tile
constexpr int RING = 6;             // B fragments in flight ahead of the MFMAs

// ---- the block, declared as locals of the kernel (a macro: as members of a struct the wave id and the tile run changed the schedules
// of all four kernels): lane / wave ids -- h: which half of the wave (K half of a fragment, 4-channel half of an 8-channel group), pl:
// row in it --, this block's run of tiles [t_begin, t_end) and tile_pos: tile t -> (image, tile row, tile column), uniform.
// Each XCD gets a contiguous eighth of the tile list and each block a contiguous run (neighbouring tiles share their halo columns in that
// XCD's L2).
#define HD_WREG_BLOCK(p, tiles_total)                                                                                       \
  const int tid = threadIdx.x, lane = tid & 63;                                                                             \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                                \
  const int h = lane >> 5, pl = lane & 31;                                                                                  \
  const int G = gridDim.x;                                                                                                  \
  const int L = hd_xcd_contiguous(blockIdx.x, G);                                                                           \
  const int t_begin = (int)((long long)L * (tiles_total) / G), t_end = (int)((long long)(L + 1) * (tiles_total) / G);       \
  const int tiles_x = ((p).Wo + TW - 1) / TW, tiles_y = ((p).Ho + TH - 1) / TH;                                             \
  auto tile_pos = [&](int t, int& n, int& ty, int& tx) {                                                                    \
    const int r1 = t / tiles_x;                                                                                             \
    tx = t - r1 * tiles_x;                                                                                                  \
    n = r1 / tiles_y;                                                                                                       \
    ty = r1 - n * tiles_y;                                                                                                  \
  }
// this lane's output pixel inside the tile (two tile rows per wave)
__device__ __forceinline__ int wreg_y0l(int wave, int lane) { return 2 * wave + ((lane >> 4) & 1); }
__device__ __forceinline__ int wreg_x0l(int lane) { return lane & 15; }

// ---- patch table entry of patch pixel pp = (py, px): py | px << 8, bit 14: beyond the patch (the last DMA piece is ragged)
__device__ __forceinline__ int wreg_patch_entry(int pp, int py, int px, int npix) { return pp < npix ? (py | (px << 8)) : 0x4000; }
// is entry E, a pixel of the patch of tile (TY, TX), inside the H x W input?  ORG: patch origin relative to the tile's first input
// pixel (-pad), SF: input pixels per output pixel (the stride).  (A macro: as a function inside issue_patch it changed how the
// compiler factors the patch base address.)
#define HD_WREG_PATCH_INSIDE(E, TY, TX, ORG, SF, H, W)                                              \
  ({                                                                                                \
    const int py_ = (E) & 0xff, px_ = ((E) >> 8) & 0x3f;                                            \
    const int iy_ = (TY) * ((SF) * TH) + (ORG) + py_, ix_ = (TX) * ((SF) * TW) + (ORG) + px_;       \
    !((E) & 0x4000) && (unsigned)iy_ < (unsigned)(H) && (unsigned)ix_ < (unsigned)(W);              \
  })

// ---- this lane's output pixel of tile (n, ty, tx): coordinates, inside the output?, element offset of its channel 0 (< 2^31: eligibility)
struct wreg_pixel { int oy, ox; bool ok; unsigned eoff; };
template <int COUT>
__device__ __forceinline__ wreg_pixel wreg_out_pixel(const ConvP& p, int y0l, int x0l, int n, int ty, int tx) {
  const int oy = ty * TH + y0l, ox = tx * TW + x0l;
  return {oy, ox, oy < p.Ho && ox < p.Wo, (unsigned)(((n * p.Ho + oy) * p.Wo + ox) * COUT)};
}

// ---- epilogue operands of 64-channel pixel PX (wreg_pixel) at SRC, indexed like the accumulator quads: Q[j] (f16x4[8]) = channels
// 8j + 4h .. + 3.  (A macro: filling the kernel's array through a reference changed the kernels' code.)
#define HD_WREG_LOAD_QUADS(Q, SRC, PX, H) \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) (Q)[j] = (PX).ok ? *reinterpret_cast<const f16x4*>((SRC) + (PX).eoff + 8 * j + 4 * (H)) : (f16x4){0, 0, 0, 0}

// ---- per-quad epilogue, EPI: 1 residual, 2 bias, 4 ReLU mask, 8 ReLU (template: as run-time flags the 64 -> 64 epilogue was 1 200
// instructions with ~60 branches and took 3 100 clocks per tile without a single store).  Order: residual, bias, mask, [sums], ReLU.
// V: float[4], one accumulator quad; R, M: f16x4 residual / mask, B: f32x4 bias of its channels.  (A macro: as functions the two
// additions came out with their operands commuted in the variants that have both.)
#define HD_WREG_EPI_OPERANDS(EPI, V, R, B, M)                                       \
  do {                                                                              \
    if ((EPI) & 1) {                                                                \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) (V)[i] += (float)(R)[i];        \
    }                                                                               \
    if ((EPI) & 2) {                                                                \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) (V)[i] += (B)[i];               \
    }                                                                               \
    if ((EPI) & 4) {                                                                \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) (V)[i] = ((float)(M)[i] > 0.f) ? (V)[i] : 0.f; \
    }                                                                               \
  } while (0)
__device__ __forceinline__ void wreg_epi_relu(float (&v)[4]) {                // EPI & 8, after the sums
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
}
// BatchNorm forward sums (sum y, sum y^2; S1, S2: float[16]) of the fp16-rounded quad G of this lane; pixels outside the output count
// as zero.  (A macro: as a function it changed the register allocation of the 128 -> 32 kernel.)
#define HD_WREG_STATS_ADD(V, OK, S1, S2, G)              \
  do {                                                   \
    const float keep = (OK) ? 1.f : 0.f;                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {      \
      const float vr = (float)(f16)(V)[i] * keep;        \
      (S1)[4 * (G) + i] += vr;                           \
      (S2)[4 * (G) + i] += vr * vr;                      \
    }                                                    \
  } while (0)
// four channels as two packed f16 pairs
__device__ __forceinline__ void wreg_pack(const float (&v)[4], unsigned (&pk)[2]) {
  const f16x2 o01 = {(f16)v[0], (f16)v[1]}, o23 = {(f16)v[2], (f16)v[3]};
  pk[0] = __builtin_bit_cast(unsigned, o01);
  pk[1] = __builtin_bit_cast(unsigned, o23);
}
// 16-byte stores: lanes l and l + 32 hold the two 4-channel halves of the same pixel's 8-channel groups g, g + 1 (pk[0], pk[1]); one
// half exchange (v_permlane32_swap) per register leaves lane l with all of group g, lane l + 32 with all of group g + 1: the result
// belongs at channel 8 (g + h)
__device__ __forceinline__ u32x4 wreg_exchange(const unsigned (&pk)[2][2]) {
  const auto q0 = __builtin_amdgcn_permlane32_swap(pk[0][0], pk[1][0], false, false);
  const auto q1 = __builtin_amdgcn_permlane32_swap(pk[0][1], pk[1][1], false, false);
  return {q0[0], q1[0], q0[1], q1[1]};
}

// ---- one partial row per block: transpose the C per-lane sums of a wave (S1[C/2] then S2[C/2], float arrays of the kernel) through LDS
// (pitch 65 floats: conflict-free both ways), lane j < C adds value j over the 32 pixel lanes of each half, then 2 C threads add the four
// waves -- fixed order throughout.  C: 64 or 32 output channels; RED_OFF: [wave][C][65] floats, RED2_OFF: [wave][C][2] floats of `lds`
// (the patch stages and any weight staging are dead).  BS (the 64 -> 64 kernel's BatchNorm-backward sums): the second row leaves as
// CF[64 + c] * (s - CF[c] * first row), CF = [mean | invstd] in LDS.  The `lane < C` guards and the extra barrier are the 32-channel
// kernel's.  (A macro: a function that takes the sums by pointer changed the code of the tile loop that accumulates them.)
#define HD_WREG_FOLD_STATS(C, BS, p, lds, RED_OFF, RED2_OFF, S1, S2, CF)                                   \
  do {                                                                                                     \
    __syncthreads();                                                                                       \
    float* red = reinterpret_cast<float*>((lds) + (RED_OFF)) + wave * ((C) * 65);                          \
    _Pragma("unroll") for (int r = 0; r < (C) / 2; ++r) {                                                  \
      red[r * 65 + lane] = (S1)[r];                                                                        \
      red[((C) / 2 + r) * 65 + lane] = (S2)[r];                                                            \
    }                                                                                                      \
    __syncthreads();                                                                                       \
    float a0 = 0.f, a1 = 0.f;                                                                              \
    if ((C) == 64 || lane < (C)) {                                                                         \
      _Pragma("unroll 8") for (int i = 0; i < 32; ++i) {                                                   \
        a0 += red[lane * 65 + i];                                                                          \
        a1 += red[lane * 65 + 32 + i];                                                                     \
      }                                                                                                    \
    }                                                                                                      \
    if ((C) < 64) __syncthreads();                                                                         \
    float* red2 = reinterpret_cast<float*>((lds) + (RED2_OFF)); /* [wave][value][half] */                  \
    if ((C) == 64 || lane < (C)) {                                                                         \
      red2[(wave * (C) + lane) * 2 + 0] = a0;                                                              \
      red2[(wave * (C) + lane) * 2 + 1] = a1;                                                              \
    }                                                                                                      \
    __syncthreads();                                                                                       \
    if (tid < 2 * (C)) {                                                                                   \
      const int v = tid >> 1, hh = tid & 1;                                                                \
      float s = 0.f;                                                                                       \
      _Pragma("unroll") for (int w4 = 0; w4 < 4; ++w4) s += red2[(w4 * (C) + v) * 2 + hh];                 \
      const int which = v >> ((C) == 64 ? 5 : 4), b = (C) == 64 ? (v >> 4) & 1 : 0, r = v & 15;            \
      const int c = 32 * b + (r & 3) + 8 * (r >> 2) + 4 * hh;                                              \
      if ((BS) && which == 1) { /* s = sum dz*m*y of channel c; its partner sum dz*m sits C/2 values below */ \
        float s0 = 0.f;                                                                                    \
        _Pragma("unroll") for (int w4 = 0; w4 < 4; ++w4) s0 += red2[(w4 * (C) + v - (C) / 2) * 2 + hh];    \
        s = (CF)[64 + c] * (s - (CF)[c] * s0);                                                             \
      }                                                                                                    \
      (p).stats[((size_t)blockIdx.x * 2 + which) * (C) + c] = s;                                           \
    }                                                                                                      \
  } while (0)

}  // namespace

// ---- host side
static inline int hd_wreg_tiles(const ConvP& p) { return p.N * hd_cdiv(p.Ho, TH) * hd_cdiv(p.Wo, TW); }
// blocks of a launch = partial-sum rows of the problem
static inline int hd_wreg_rows(const ConvP& p) {
  const int t = hd_wreg_tiles(p);
  return t < 256 ? t : 256;
}
// the EPI bits of a problem
static inline int hd_wreg_epi(const ConvP& p) { return (p.res ? 1 : 0) | (p.bias ? 2 : 0) | (p.mask ? 4 : 0) | (p.act == HD_ACT_RELU ? 8 : 0); }
// launch KERNEL<STATS, EPI>(p, tiles) with the problem's EPI bits, STATS = ON with p.stats, OFF without (16 x 2 instantiations)
#define HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, E, p, s)                                                                  \
  case E:                                                                                                              \
    if ((p).stats) hipLaunchKernelGGL((KERNEL<ON, E>), dim3(hd_wreg_rows(p)), dim3(256), 0, s, p, hd_wreg_tiles(p));   \
    else hipLaunchKernelGGL((KERNEL<OFF, E>), dim3(hd_wreg_rows(p)), dim3(256), 0, s, p, hd_wreg_tiles(p));            \
    break;
#define HD_WREG_LAUNCH_EPI(KERNEL, OFF, ON, p, s)                                                                                              \
  switch (hd_wreg_epi(p)) {                                                                                                                    \
    HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 0, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 1, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 2, p, s)   \
    HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 3, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 4, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 5, p, s)   \
    HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 6, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 7, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 8, p, s)   \
    HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 9, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 10, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 11, p, s) \
    HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 12, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 13, p, s) HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 14, p, s) \
    HD_WREG_LAUNCH_CASE(KERNEL, OFF, ON, 15, p, s)                                                                                              \
  }
