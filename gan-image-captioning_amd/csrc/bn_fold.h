// BatchNorm batch statistics arrive as per-channel sums in a few REPLICAS ([nrep][2][C] f32: the producing convolution's workgroups add
// into replica b % nrep so that few atomics share an address); every consumer folds them per channel.  Shared by the kernels that normalise
// on load (gemm.hip, conv3x3.hip, conv1x1_stream.hip, conv1x1_panel.hip, conv1x1_pix.hip, conv_b2b.hip) and by encoder.hip's bn_act family.
#pragma once
#include "common.h"

namespace gic {

constexpr float kBnEps = 1e-5f;       // nn.BatchNorm2d default

// Sum / sum of squares of channel c over the replicas: eight independent pairs of loads in flight per round trip (a load / add loop
// waits for each replica in turn: measured as one L2 round trip per replica in every workgroup's prologue); replicas past nrep
// re-read the last one with weight 0.
__device__ __forceinline__ void fold_replicas(const float* stats, int nrep, int C, int c, float& s1, float& s2) {
  s1 = s2 = 0.f;
  for (int r0 = 0; r0 < nrep; r0 += 8) {
    float a[8], q[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const long rr = min(r0 + r, nrep - 1);
      a[r] = stats[rr * 2 * C + c];
      q[r] = stats[rr * 2 * C + C + c];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float wgt = r0 + r < nrep ? 1.f : 0.f;
      s1 += wgt * a[r]; s2 += wgt * q[r];
    }
  }
}

// mean and 1 / sqrt(var + eps) of channel c of C from the replicated sums over 1 / inv_count rows (biased variance, clamped at 0)
__device__ __forceinline__ void bn_moments(const float* stats, int nrep, int C, int c, float inv_count, float& mean, float& rstd) {
  float s1, s2;
  fold_replicas(stats, nrep, C, c, s1, s2);
  const float m = s1 * inv_count;
  const float var = fmaxf(s2 * inv_count - m * m, 0.f);
  mean = m;
  rstd = rsqrtf(var + kBnEps);
}

// [scale, shift] of channel c (a kernel that loads gamma and beta at a point of its own takes bn_moments and forms the two itself)
__device__ __forceinline__ void bn_scale_shift(const float* stats, int nrep, int C, int c, float inv_count, const float* gamma, const float* beta, float& scale, float& shift) {
  const float gam = gamma[c], bet = beta[c];                             // in flight together with the replicas
  float mean, rstd;
  bn_moments(stats, nrep, C, c, inv_count, mean, rstd);
  const float sc = gam * rstd;
  scale = sc;
  shift = bet - mean * sc;
}

// eight consecutive channels' [scale, shift] pairs of a coefficient table (coef = the first one's, 16-byte aligned) as four 16-byte reads
__device__ __forceinline__ void bn_unpack8(const float* coef, float (&scl)[8], float (&sft)[8]) {
  const float4* cp = (const float4*)coef;
  const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3];
  scl[0] = c0.x; scl[1] = c0.z; scl[2] = c1.x; scl[3] = c1.z; scl[4] = c2.x; scl[5] = c2.z; scl[6] = c3.x; scl[7] = c3.z;
  sft[0] = c0.y; sft[1] = c0.w; sft[2] = c1.y; sft[3] = c1.w; sft[4] = c2.y; sft[5] = c2.w; sft[6] = c3.y; sft[7] = c3.w;
}

// BatchNorm + ReLU of eight bf16 values of those channels
__device__ __forceinline__ bf16x8 bn_relu8(bf16x8 v, const float (&scl)[8], const float (&sft)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (bf16_t)fmaxf((float)v[e] * scl[e] + sft[e], 0.f);
  return v;
}

}  // namespace gic
