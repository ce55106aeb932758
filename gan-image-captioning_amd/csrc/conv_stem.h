// Streaming stem convolution of the trunk (conv_stem.hip): launcher shared with gemm.hip's convolution dispatch.
#pragma once
#include "gemm.h"

namespace gic {

struct StemDesc : ConvBase {
  int Nimg, H, W, Ho, Wo;
  int ranges, rows_per_range;            // workgroups per image, output rows per workgroup
};

struct StemPlan { StemDesc d; unsigned grid; size_t lds; };

// Qualifies: window 7 x 8 over a pre-padded NHWC4 bf16 image, stride 2, 64 output channels, output rows of <= 128 pixels, BatchNorm-sum
// epilogue.
bool select_conv_stem(const GemmDesc& d, StemPlan& p);
bool launch_conv_stem(const StemPlan& p, hipStream_t stream);

}  // namespace gic
