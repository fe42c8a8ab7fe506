// The 64-deep instances of the implicit-GEMM family (conv_igemm_body.h, BK = 64): full 128-byte-line DMA pieces, one barrier per
// 16 MFMAs, three LDS stages in the deep variants.  The dispatcher sends Cin % 64 == 0 here (per source when there are two).
#include "conv_igemm_body.h"

void hd_conv_launch_bk64(ConvP& p, int bm, int bn, bool deep, hipStream_t s) { conv_igemm_launch<64>(p, bm, bn, deep, s); }

bool hd_conv_launch_bk64_multi(ConvMulti& mp, int bm, int bn, bool deep, hipStream_t s) { return conv_igemm_launch_multi<64>(mp, bm, bn, deep, s); }
