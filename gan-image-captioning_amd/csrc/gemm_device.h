// Device helpers shared by the kernels built on 16x16 MFMA tiles (gemm.hip's two kernels, the dynamic-LDS trunk convolutions, the
// discriminator's redrop kernel): the swizzle of the LDS image, the TM x TN MFMA block, the highway gate and keep draw, the implicit-GEMM
// convolution addressing.  No kernel lives here.  The helpers take and return numbers, never an LDS pointer: a helper that did (the
// fragment read itself, the staged C tile's column sums and row stores) changed the scheduling of the kernels it was inlined into.
#pragma once
#include "common.h"

namespace gic {

// ---- the k-contiguous LDS image with 128-byte rows: the 16-byte chunk index is XORed with (row >> 1) & 7 (bank conflicts of the
// fragment reads).  A reader finds logical chunk c of a row at byte row * 128 + swz_chunk(row, c); an LDS-DMA writer fills physical slot
// tid & 7 of row tid >> 3 (+ a multiple of 16 rows), which holds the logical chunk swz_dma_chunk(tid).
__device__ __forceinline__ int swz_chunk(const int row, const int chunk) { return (chunk ^ ((row >> 1) & 7)) << 4; }
__device__ __forceinline__ int swz_dma_chunk(const int tid) { return (tid & 7) ^ ((tid >> 4) & 7); }

// acc[i][j] += fa[i] x fb[j] over one 32-deep K step (v_mfma_f32_16x16x32_bf16)
template <int TM, int TN>
__device__ __forceinline__ void mfma_block(f32x4 (&acc)[TM][TN], const bf16x8 (&fa)[TM], const bf16x8 (&fb)[TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
}

// ---- highway (discriminator.py:53-58): y = sig(h) relu(h) + (1 - sig(h)) x
__device__ __forceinline__ float highway_gate(const float h, const float x) {
  const float sg = 1.f / (1.f + expf(-h));
  return sg * fmaxf(h, 0.f) + (1.f - sg) * x;
}
// The dropout keep flags of column n for the 4 consecutive rows 4 quad .. 4 quad + 3 of an [M, N] output: ONE Philox4x32 call
__device__ __forceinline__ void highway_keep4(const uint64_t seed, const uint64_t stream, const uint64_t quad, const int N, const int n,
                                              const float drop_p, float (&keep)[4]) {
  uint32_t r[4];
  Philox::gen4(seed, stream, quad * (uint64_t)N + (uint64_t)n, r[0], r[1], r[2], r[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) keep[i] = Philox::u01(r[i]) >= drop_p ? 1.f : 0.f;
}

// ---- implicit-GEMM convolution, k = (r * KW + s) * Cin + c.
// Output row m of an [Nimg, Ho, Wo] map -> its window's top-left input pixel (hi0, wi0) and the pixel index of that corner in the
// [Nimg, H, W] input, in the index type T of the caller's addressing.  A row that is not `ok` (past M) gets an hi0 that never validates.
template <typename T> struct ConvOrigin { int hi0, wi0; T pix; };
template <typename T>
__device__ __forceinline__ ConvOrigin<T> conv_origin(const int m, const bool ok, const int Ho, const int Wo, const int H, const int W,
                                                     const int stride, const int pad) {
  const int mm = ok ? m : 0;
  const int wo = mm % Wo, t = mm / Wo;
  const int ho = t % Ho, n = t / Ho;
  ConvOrigin<T> o;
  o.hi0 = ok ? ho * stride - pad : -(1 << 28);
  o.wi0 = wo * stride - pad;
  o.pix = ((T)n * H + o.hi0) * W + o.wi0;
  return o;
}
// (r, s, c) of a thread's chunk, advanced by one K tile of BK channels
__device__ __forceinline__ void conv_tap_advance(int& r, int& s, int& c, const int BK, const int Cin, const int KW) {
  c += BK;
  while (c >= Cin) {
    c -= Cin;
    if (++s == KW) { s = 0; ++r; }
  }
}

}  // namespace gic
