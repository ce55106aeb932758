// conv3 -> bn3 + shortcut + ReLU -> next conv1 in one launch (conv_b2b.hip); see there.
#pragma once
#include "common.h"

namespace gic {

struct B2bDesc {
  const void* y2; const void* w3; const void* res; const void* w1n;     // bf16: [M, C2], [4 C2, C2], [M, 4 C2], [C1N, 4 C2]
  void* out; void* y1n;                                                  // bf16: [M, 4 C2] block output, [M, C1N] raw conv1_next output
  const float* stats2; const float* gamma2; const float* beta2;          // BatchNorm of y2 (bn2): column sums [nrep2][2][C2]
  const float* stats3; const float* gamma3; const float* beta3;          // bn3: sums of conv3's output from the statistics-only pass
  const float* res_stats; const float* res_gamma; const float* res_beta; // the projection shortcut's BatchNorm, or null (identity)
  float* stats1;                                                         // [nrep1][2][C1N]: conv1_next's column sums are ADDED
  int nrep2, nrep3, res_nrep, nrep1;
  float inv_count;                                                       // 1 / M (all four BatchNorms normalise over the same rows)
  int M;
  unsigned y2_bytes, res_bytes, y1n_bytes = 0;
};

struct B2bPlan { B2bDesc d; int C2, C1N; bool ident; int tiles, per_cu; size_t lds; };   // conv_b2b_kernel<C2, C1N, IDENT>, grid = min(tiles, CUs * per_cu)

// The shapes the kernel is instantiated for and can address: what gic_conv_b2b_supported answers and select_conv_b2b starts with
bool conv_b2b_shape_ok(long rows, int C2, int C1N);
// false: no instantiation for these shapes or operands (the caller runs the separate launches).  Fills d's byte extents.
bool select_conv_b2b(const B2bDesc& d, int C2, int C1N, B2bPlan& p);
bool launch_conv_b2b(const B2bPlan& p, hipStream_t stream);

}  // namespace gic
