// The 32-deep instances of the implicit-GEMM family (conv_igemm_body.h, BK = 32): half-line DMA pieces, four LDS stages in the
// deep variants.  Any Cin % 8 == 0 (per-lane taps when Cin % 32 != 0) and the 32-wide N tile run here.
#include "conv_igemm_body.h"

void hd_conv_launch_bk32(ConvP& p, int bm, int bn, bool deep, hipStream_t s) { conv_igemm_launch<32>(p, bm, bn, deep, s); }

bool hd_conv_launch_bk32_multi(ConvMulti& mp, int bm, int bn, bool deep, hipStream_t s) { return conv_igemm_launch_multi<32>(mp, bm, bn, deep, s); }
