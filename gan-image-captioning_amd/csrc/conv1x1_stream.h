// Streaming shallow-K 1x1 convolution of the trunk (conv1x1_stream.hip): launcher shared with gemm.hip's convolution dispatch.
#pragma once
#include "gemm.h"

namespace gic {

struct StreamDesc : ConvBase {
  int share_a;
  int stats_only;                      // column sums only: no C stores
  int tiles_m, tiles_n, groups;        // row tiles, output-channel tiles, workgroups per output-channel tile (grid = groups * tiles_n)
};

struct StreamPlan { StreamDesc d; int BN, KT; bool abn, stats; unsigned grid; size_t lds; };   // conv1x1_stream_kernel<BN, KT, ABN, STATS>

// Qualifies: 1x1 / stride 1, K = 64 or 128, bf16, BatchNorm-sum epilogue, optional BatchNorm + ReLU of the input on load, >= 1024 output
// tiles.
bool select_conv1x1_stream(const GemmDesc& d, StreamPlan& p);
bool launch_conv1x1_stream(const StreamPlan& p, hipStream_t stream);

}  // namespace gic
