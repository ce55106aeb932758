// Pixel-resident 1x1 convolution of the trunk's small maps (conv1x1_pix.hip): launcher shared with gemm.hip's convolution dispatch.
#pragma once
#include "gemm.h"

namespace gic {

struct PixDesc : ConvBase {
  int tiles_m, per_group;              // row tiles of 128 pixels; 64-channel tiles per workgroup (grid = tiles_m * groups)
  unsigned c_bytes;
};

struct PixPlan { PixDesc d; int K, NSTG; bool turn; unsigned grid; size_t lds; };   // conv1x1_pix_kernel<K, NSTG, TURN>

// Qualifies: 1x1 / stride 1, K = 256 | 512, N >= 512 and a multiple of 64, at least 128 rows, bf16, BatchNorm-sum epilogue, BatchNorm + ReLU
// of the input on load.
bool select_conv1x1_pix(const GemmDesc& d, PixPlan& p);
bool launch_conv1x1_pix(const PixPlan& p, hipStream_t stream);

}  // namespace gic
