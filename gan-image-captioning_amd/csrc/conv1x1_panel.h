// A-panel-resident 1x1 convolution of the trunk (conv1x1_panel.hip): launcher shared with gemm.hip's convolution dispatch.
#pragma once
#include "gemm.h"

namespace gic {

struct PanelDesc : ConvBase {
  int share_a;
  int tiles_m, tiles_n, groups, per_group;   // row tiles, 64-wide output-channel tiles, groups of them, tiles per group
};

struct PanelPlan { PanelDesc d; int KT; bool abn; unsigned grid; size_t lds; };   // conv1x1_panel_kernel<KT, ABN>

// Qualifies: 1x1 / stride 1, K = 256, N >= 512 and a multiple of 64, bf16, BatchNorm-sum epilogue, optional BatchNorm + ReLU of the input on
// load.
bool select_conv1x1_panel(const GemmDesc& d, PanelPlan& p);
bool launch_conv1x1_panel(const PanelPlan& p, hipStream_t stream);

}  // namespace gic
