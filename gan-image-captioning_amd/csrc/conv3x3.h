// Patch-resident 3x3 convolution of the trunk (conv3x3.hip): launcher shared with gemm.hip's convolution dispatch.
#pragma once
#include "gemm.h"

namespace gic {

// Everything the kernel reads from its arguments, compact and in one struct: the scalar loads of a few adjacent cache lines leave in one
// batch at the top (fields of the 384-byte GemmDesc, fetched where first used, cost the prologue five serial round trips: ~1.2 us).
struct PatchDesc : ConvBase {
  int H, W, Cin;
  int tiles_m;              // row tiles
  int tiles_n;              // > 0: output-channel tiles, and those of one row tile are neighbours on an XCD; 0: the row tiles of a channel tile are
  int tpi;                  // > 0: tiles never cross an image (tpi tiles per image, the last one short); 0: 128 consecutive rows of M
  int nchunks;              // Cin / 64
};

struct PatchPlan { PatchDesc d; int BN, P; bool multi, abn; unsigned grid; size_t lds; };   // conv3x3_patch_kernel<BN, P, MULTI, ABN>

// Qualifies: 3x3 / stride 1 / pad 1, bf16 NHWC, Cin % 64 == 0, BatchNorm-sum epilogue, optional BatchNorm + ReLU of the input on load, a
// patch that fits one of the instantiated buffers.
bool select_conv3x3_patch(const GemmDesc& d, PatchPlan& p);
bool launch_conv3x3_patch(const PatchPlan& p, hipStream_t stream);

}  // namespace gic
