// Output dropout of the caption decoder (gicap.h gic_decoder_dropout; gic_hidden_dropout, gic_hidden_dropout_bwd and the
// gic_*_forward_*_drop entry points of teacher_forced.hip): the LSTM output hout [B, Tmax, H] is dropped in front of the vocabulary
// projection; the recurrence keeps the undropped h.
//   keep[b, t, h]  = u[b, t, h] >= p                      (the convention of highway_keep4)
//   hdrop[b, t, :] = keep ? from_f32(hout * s) : 0        s = 1.0f / (1.0f - p), formed in f32 on the host
//   dhout[b, t, :] = (t < lengths[b] && keep) ? dhout * s : 0      (in place; replaces zero_past_length on the dropout path)
// The map from element to draw: element (r = b * Tmax + t, h) has the flat index i = r * H + h and takes lane i & 3 of
// Philox::gen(seed, kGenDropStream, i >> 2); with keep_u (f32 [B, Tmax, H]) u is read at i instead.  The mask is a function of
// (seed, p, i) alone: the backward regenerates it and nothing is stored for it, and a kernel that covers the B rows of one step t
// (scheduled sampling decides the next input from the dropped logits of step t) draws the bits the all-rows kernel draws.
// Both kernels have a 16-byte form (H % 4 == 0 in f32, H % 8 == 0 in bf16, 16-byte aligned bases: every row then starts on a 16-byte
// boundary and a piece of 4 elements is one Philox call) and a scalar form for every other H or base.  No atomics, no reductions: the
// same inputs give the same bits in either mode.
#include "../../include/gicap.h"
#include "decoder_step.h"
#include "kernels.h"

namespace gic {
namespace {

constexpr uint64_t kGenDropStream = (uint64_t)0x6764726F << 32;    // "gdro"

// the four uniforms of the quad of elements 4 q .. 4 q + 3
__device__ __forceinline__ void drop_u4(const float* __restrict__ keep_u, bool u_vec, uint64_t seed, long q, float (&u)[4]) {
  if (keep_u) {
    if (u_vec) {
      Vec16<float>::load(keep_u + 4 * q, u);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = keep_u[4 * q + j];
    }
    return;
  }
  uint32_t r0, r1, r2, r3;
  Philox::gen4(seed, kGenDropStream, (uint64_t)q, r0, r1, r2, r3);
  u[0] = Philox::u01(r0); u[1] = Philox::u01(r1); u[2] = Philox::u01(r2); u[3] = Philox::u01(r3);
}

// the uniform of element i
__device__ __forceinline__ float drop_u1(const float* __restrict__ keep_u, uint64_t seed, long i) {
  if (keep_u) return keep_u[i];
  uint32_t r0, r1, r2, r3;
  Philox::gen4(seed, kGenDropStream, (uint64_t)(i >> 2), r0, r1, r2, r3);
  const int lane = (int)(i & 3);
  return Philox::u01(lane == 0 ? r0 : (lane == 1 ? r1 : (lane == 2 ? r2 : r3)));
}

// row r of the n-th selected row: every row (step < 0) or the rows b * Tmax + step
__device__ __forceinline__ long drop_row(long n, int Tmax, int step) { return step < 0 ? n : n * Tmax + step; }

// 16-byte form: one work item = NV consecutive elements of a row (NV / 4 quads); nsel rows of H / NV items
template <typename TA>
__global__ void hidden_dropout_fwd_vec_kernel(const TA* x, TA* y, const float* __restrict__ keep_u, bool u_vec, uint64_t seed, float p,
                                              float s, long nsel, int H, int Tmax, int step) {
  constexpr int NV = Vec16<TA>::NV;
  const int per_row = H / NV;
  const long total = nsel * per_row;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
    const long i = drop_row(g / per_row, Tmax, step) * H + (long)(g % per_row) * NV;      // i % 4 == 0: H % 4 == 0
    float v[NV];
    Vec16<TA>::load(x + i, v);
#pragma unroll
    for (int k = 0; k < NV / 4; ++k) {
      float u[4];
      drop_u4(keep_u, u_vec, seed, (i >> 2) + k, u);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = u[j] >= p ? v[4 * k + j] * s : 0.f;
    }
    Vec16<TA>::store(y + i, v);
  }
}

template <typename TA>
__global__ void hidden_dropout_fwd_kernel(const TA* x, TA* y, const float* __restrict__ keep_u, uint64_t seed, float p, float s, long nsel,
                                          int H, int Tmax, int step) {
  const long total = nsel * H;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
    const long i = drop_row(g / H, Tmax, step) * H + g % H;
    y[i] = drop_u1(keep_u, seed, i) >= p ? from_f32<TA>(to_f32<TA>(x[i]) * s) : from_f32<TA>(0.f);
  }
}

// in place on dhout f32 [B, Tmax, H]; a row past its caption's length is zeroed without a draw
__global__ void hidden_dropout_bwd_vec_kernel(float* dhout, const int32_t* __restrict__ lengths, const float* __restrict__ keep_u, bool u_vec,
                                              uint64_t seed, float p, float s, long rows, int H, int Tmax) {
  const int per_row = H / 4;
  const long total = rows * per_row;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
    const long r = g / per_row;
    const long i = r * H + (long)(g % per_row) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if ((int)(r % Tmax) < lengths[r / Tmax]) {
      float u[4];
      Vec16<float>::load(dhout + i, v);
      drop_u4(keep_u, u_vec, seed, i >> 2, u);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = u[j] >= p ? v[j] * s : 0.f;
    }
    Vec16<float>::store(dhout + i, v);
  }
}

__global__ void hidden_dropout_bwd_kernel(float* dhout, const int32_t* __restrict__ lengths, const float* __restrict__ keep_u, uint64_t seed,
                                          float p, float s, long rows, int H, int Tmax) {
  const long total = rows * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / H;
    const bool live = (int)(r % Tmax) < lengths[r / Tmax];
    dhout[i] = live && drop_u1(keep_u, seed, i) >= p ? dhout[i] * s : 0.f;
  }
}

dim3 drop_grid(long items) {
  const long blocks = (items + 255) / 256;
  return dim3((unsigned)(blocks > 2048 ? 2048 : (blocks < 1 ? 1 : blocks)));
}

bool aligned16(const void* a, const void* b = nullptr) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

float drop_scale(float p) { return 1.0f / (1.0f - p); }

int drop_check_p(float p, const char* who) {
  GIC_CHECK_ARG(p > 0.f && p < 1.f, "%s: p must be in (0, 1)", who);      // false for NaN
  return GIC_OK;
}

}  // namespace

int hidden_dropout_fwd(int dt, const void* x, void* y, const float* keep_u, uint64_t seed, float p, int B, int Tmax, int H, int step,
                       hipStream_t stream) {
  const long nsel = step < 0 ? (long)B * Tmax : (long)B;
  const float s = drop_scale(p);
  const int nv = dt == DT_F32 ? 4 : 8;
  const bool u_vec = aligned16(keep_u);
  if (H % nv == 0 && aligned16(x, y)) {
    const dim3 grid = drop_grid(nsel * (H / nv));
    if (dt == DT_F32)
      hipLaunchKernelGGL((hidden_dropout_fwd_vec_kernel<float>), grid, dim3(256), 0, stream, (const float*)x, (float*)y, keep_u, u_vec, seed, p, s,
                         nsel, H, Tmax, step);
    else
      hipLaunchKernelGGL((hidden_dropout_fwd_vec_kernel<bf16_t>), grid, dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)y, keep_u, u_vec, seed, p,
                         s, nsel, H, Tmax, step);
  } else {
    const dim3 grid = drop_grid(nsel * H);
    if (dt == DT_F32)
      hipLaunchKernelGGL((hidden_dropout_fwd_kernel<float>), grid, dim3(256), 0, stream, (const float*)x, (float*)y, keep_u, seed, p, s, nsel, H,
                         Tmax, step);
    else
      hipLaunchKernelGGL((hidden_dropout_fwd_kernel<bf16_t>), grid, dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)y, keep_u, seed, p, s, nsel, H,
                         Tmax, step);
  }
  GIC_CHECK_LAUNCH("hidden_dropout_fwd");
  return GIC_OK;
}

int hidden_dropout_bwd(float* dhout, const int32_t* lengths, const float* keep_u, uint64_t seed, float p, int B, int Tmax, int H,
                       hipStream_t stream) {
  const long rows = (long)B * Tmax;
  const float s = drop_scale(p);
  if (H % 4 == 0 && aligned16(dhout))
    hipLaunchKernelGGL(hidden_dropout_bwd_vec_kernel, drop_grid(rows * (H / 4)), dim3(256), 0, stream, dhout, lengths, keep_u, aligned16(keep_u),
                       seed, p, s, rows, H, Tmax);
  else
    hipLaunchKernelGGL(hidden_dropout_bwd_kernel, drop_grid(rows * H), dim3(256), 0, stream, dhout, lengths, keep_u, seed, p, s, rows, H, Tmax);
  GIC_CHECK_LAUNCH("hidden_dropout_bwd");
  return GIC_OK;
}

int drop_check(const gic_decoder_dropout* d, const char* who) {
  GIC_CHECK_ARG(d, "%s: null dropout", who);
  GIC_PROPAGATE(drop_check_p(d->p, who));
  GIC_CHECK_ARG(d->hdrop, "%s: hdrop is null", who);
  GIC_CHECK_ARG(aligned16(d->hdrop), "%s: hdrop must be 16-byte aligned", who);
  return GIC_OK;
}

}  // namespace gic

using namespace gic;

extern "C" {

int gic_hidden_dropout(const void* x, int dtype, int64_t rows, int32_t H, float p, uint64_t seed, const float* keep_u, void* y,
                       void* stream) {
  GIC_CHECK_ARG(x && y, "hidden_dropout: null argument");
  GIC_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16, "hidden_dropout: bad dtype");
  GIC_CHECK_ARG(rows > 0 && rows <= INT32_MAX && H > 0, "hidden_dropout: bad dims");
  GIC_PROPAGATE(drop_check_p(p, "hidden_dropout"));
  return hidden_dropout_fwd(dtype, x, y, keep_u, seed, p, (int)rows, 1, H, -1, (hipStream_t)stream);
}

int gic_hidden_dropout_bwd(float* dhout, const int32_t* lengths, int32_t B, int32_t Tmax, int32_t H, float p, uint64_t seed,
                           const float* keep_u, void* stream) {
  GIC_CHECK_ARG(dhout && lengths, "hidden_dropout_bwd: null argument");
  GIC_CHECK_ARG(B > 0 && Tmax > 0 && H > 0, "hidden_dropout_bwd: bad dims");
  GIC_PROPAGATE(drop_check_p(p, "hidden_dropout_bwd"));
  return hidden_dropout_bwd(dhout, lengths, keep_u, seed, p, B, Tmax, H, (hipStream_t)stream);
}

}  // extern "C"
