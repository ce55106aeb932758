// Image-conditioned discriminator (projection form, Miyato & Koyama 2018): the match term between a caption's highway output y and its
// image's projection q = img_proj(pooled trunk feature), and its backward.  No reference counterpart.
//
//   logits[m] (+)= s <y[m, :F], q[m / R, :]>            s = F^-1/2, row m = b R + r, y = state->ydrop (what feature2out consumes)
//   logits[m] (+)= s <y[m, :F], q[q_index[b], :]>       the grouped form (inference only): caption b against any of q's q_rows rows
//   dydrop[m, n]  = s g[m] q[b, n]                      (f32, pad columns F .. Fp-1 zero; the feature2out input-gradient product of
//                                                        disc_bwd_t then accumulates onto it)
//   d_q[b, n]     = s sum_r g[b R + r] y[b R + r, n]    (r in index order: no atomics, the same bits in either mode)
// Both kernels are streams over y [B*R, Fp] (compute dtype) with nothing to reuse but q[b] (F floats per caption).
#include "../../include/gicap.h"
#include "kernels.h"

namespace gic {
namespace {

// ---- forward.  grid = (captions, row groups); a workgroup stages q[b] once in LDS (zero beyond F) for all its rows; a wave owns a row at
// a time: 16-byte loads along the row (64 lanes = 1 KiB per pass), a wave-level sum, lane 0 writes the logit.
// q_index (NULL = the identity): caption b reads row q_index[b] of q's q_rows rows; an index outside [0, q_rows) is never dereferenced, the
// caption's rows get NaN (workgroup-uniform).  K captions of one image = K consecutive workgroups staging the same row from L2.
template <typename TA>
__global__ __launch_bounds__(256) void disc_match_fwd_kernel(const TA* __restrict__ y, const float* __restrict__ q, const int32_t* __restrict__ q_index,
                                                               int q_rows, float scale, int accumulate, float* __restrict__ logits, int R, int F, int Fp,
                                                               int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) float qs[];     // [Fp]
  constexpr int E = 16 / (int)sizeof(TA);                         // elements per 16-byte load
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qb = q_index ? q_index[b] : b;
  const bool in_range = (unsigned)qb < (unsigned)q_rows;
  for (int n = threadIdx.x; n < Fp; n += 256) qs[n] = n < F && in_range ? q[(long)qb * F + n] : 0.f;
  __syncthreads();
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = r0 + rows_per_block < R ? r0 + rows_per_block : R;
  for (int r = r0 + w; r < r1; r += 4) {                          // wave-uniform
    const long m = (long)b * R + r;
    const TA* row = y + m * Fp;
    float acc = 0.f;
    for (int c = lane * E; c < Fp; c += 64 * E) {
      __attribute__((aligned(16))) TA v[E];
      *(float4*)v = *(const float4*)(row + c);
#pragma unroll
      for (int e = 0; e < E; ++e) acc += to_f32<TA>(v[e]) * qs[c + e];
    }
    acc = wave_sum(acc);
    if (lane == 0) logits[m] = in_range ? (accumulate ? logits[m] : 0.f) + scale * acc : __builtin_nanf("");
  }
}

// ---- backward.  One thread per (caption, 4 columns) walks the caption's R rows in index order: per row one 8- / 16-byte load of y, one
// 16-byte store of dydrop (a wave covers 256 consecutive columns: 1 KiB stores), g[m] wave-uniform.  grid = (column groups / 64, captions).
template <typename TA>
__global__ __launch_bounds__(64) void disc_match_bwd_kernel(const TA* __restrict__ y, const float* __restrict__ q, const float* __restrict__ g,
                                                              float scale, float* __restrict__ dydrop, float* __restrict__ d_q, int R, int F, int Fp) {
  const int b = blockIdx.y;
  const int n0 = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (n0 >= Fp) return;
  float sq[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) sq[e] = n0 + e < F ? scale * q[(long)b * F + n0 + e] : 0.f;
  const long m0 = (long)b * R;
#pragma unroll 8
  for (int r = 0; r < R; ++r) {
    const long o = (m0 + r) * Fp + n0;
    const float gm = g[m0 + r];
    __attribute__((aligned(16))) TA v[4];
    if (sizeof(TA) == 4) *(float4*)v = *(const float4*)(y + o);
    else *(float2*)v = *(const float2*)(y + o);
    float out[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      out[e] = n0 + e < F ? gm * sq[e] : 0.f;
      acc[e] += gm * to_f32<TA>(v[e]);
    }
    *(float4*)(dydrop + o) = make_float4(out[0], out[1], out[2], out[3]);
  }
  if (d_q) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n0 + e < F) d_q[(long)b * F + n0 + e] = scale * acc[e];
  }
}

// The weighted mix of two evaluations of the D loss: a = d(real, fake), b = d(real, wrong)
//   losses_a[1] = (1 - w) losses_a[1] + w losses_b[1];   dd_real_a = (1 - w) dd_real_a + w dd_real_b;   dd_fake_a *= 1 - w;   dd_fake_b *= w
__global__ void gan_losses_mix_kernel(float w, long n, float* __restrict__ losses_a, const float* __restrict__ losses_b, float* __restrict__ dd_real_a,
                                      float* __restrict__ dd_fake_a, const float* __restrict__ dd_real_b, float* __restrict__ dd_fake_b) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) losses_a[1] = (1.f - w) * losses_a[1] + w * losses_b[1];
  if (i < n && dd_real_a) {
    dd_real_a[i] = (1.f - w) * dd_real_a[i] + w * dd_real_b[i];
    dd_fake_a[i] = (1.f - w) * dd_fake_a[i];
    dd_fake_b[i] = w * dd_fake_b[i];
  }
}

int check_match_dims(const gic_disc_dims* d, const char* what) {
  GIC_CHECK_ARG(d, "%s: null dims", what);
  GIC_CHECK_ARG(d->B >= 1 && d->R >= 1, "%s: B=%d and R=%d must be >= 1", what, d->B, d->R);
  GIC_CHECK_ARG(d->dtype == DT_F32 || d->dtype == DT_BF16, "%s: bad dtype", what);
  GIC_CHECK_ARG(d->F >= 1 && d->Fp >= d->F && d->Fp % 8 == 0, "%s: Fp=%d must be >= F=%d >= 1 and a multiple of 8", what, d->Fp, d->F);
  GIC_CHECK_ARG((size_t)d->Fp * sizeof(float) <= 64 * 1024, "%s: Fp=%d exceeds the LDS staging of q (16384 floats)", what, d->Fp);
  return GIC_OK;
}

// The one launch of the match forward (gic_disc_match_fwd: the identity index over B rows of q; gic_disc_match_fwd_grouped).
int launch_match_fwd(const gic_disc_dims* dims, const void* ydrop, const float* q, int q_rows, const int32_t* q_index, float scale, int accumulate,
                     float* logits, hipStream_t stream, const char* what) {
  const int B = dims->B, R = dims->R, F = dims->F, Fp = dims->Fp;
  // rows per workgroup (a multiple of its four waves): halved until the grid has 512 workgroups, so that q[b] is staged as seldom as the
  // device's occupancy allows (cfg2: 8 rows, two per wave)
  int rpb = R;
  while (rpb > 4 && (long)B * cdiv(R, rpb) < 512) rpb = (rpb + 1) / 2;
  rpb = (rpb + 3) / 4 * 4;
  const dim3 grid(B, cdiv(R, rpb));
  const size_t lds = (size_t)Fp * sizeof(float);
  if (dims->dtype == DT_F32)
    hipLaunchKernelGGL((disc_match_fwd_kernel<float>), grid, dim3(256), lds, stream, (const float*)ydrop, q, q_index, q_rows, scale, accumulate,
                       logits, R, F, Fp, rpb);
  else
    hipLaunchKernelGGL((disc_match_fwd_kernel<bf16_t>), grid, dim3(256), lds, stream, (const bf16_t*)ydrop, q, q_index, q_rows, scale, accumulate,
                       logits, R, F, Fp, rpb);
  GIC_CHECK_LAUNCH(what);
  return GIC_OK;
}

}  // namespace

int disc_match_bwd(int dt, const void* ydrop, const float* q, const float* g, float scale, float* dydrop, float* d_q, int B, int R, int F,
                   int Fp, hipStream_t stream) {
  GIC_CHECK_ARG(ydrop && q && g && dydrop, "disc_match_bwd: null argument");
  GIC_CHECK_ARG(((((uintptr_t)ydrop) | ((uintptr_t)dydrop)) & 15) == 0, "disc_match_bwd: ydrop / dydrop must be 16-byte aligned");
  const dim3 grid(cdiv(Fp / 4, 64), B);
  if (dt == DT_F32)
    hipLaunchKernelGGL((disc_match_bwd_kernel<float>), grid, dim3(64), 0, stream, (const float*)ydrop, q, g, scale, dydrop, d_q, R, F, Fp);
  else
    hipLaunchKernelGGL((disc_match_bwd_kernel<bf16_t>), grid, dim3(64), 0, stream, (const bf16_t*)ydrop, q, g, scale, dydrop, d_q, R, F, Fp);
  GIC_CHECK_LAUNCH("disc_match_bwd");
  return GIC_OK;
}

}  // namespace gic

using namespace gic;

extern "C" {

int gic_disc_match_fwd(const gic_disc_dims* dims, const gic_disc_state* state, const float* q, float scale, int accumulate, float* logits,
                       void* stream) {
  GIC_PROPAGATE(check_match_dims(dims, "disc_match_fwd"));
  GIC_CHECK_ARG(state && q && logits, "disc_match_fwd: null argument");
  GIC_CHECK_ARG(state->ydrop, "disc_match_fwd: null state buffer (ydrop)");
  GIC_CHECK_ARG((((uintptr_t)state->ydrop) & 15) == 0, "disc_match_fwd: ydrop must be 16-byte aligned");
  GIC_CHECK_ARG(scale == scale, "disc_match_fwd: scale is NaN");
  return launch_match_fwd(dims, state->ydrop, q, dims->B, nullptr, scale, accumulate, logits, (hipStream_t)stream, "disc_match_fwd");
}

int gic_disc_match_fwd_grouped(const gic_disc_dims* dims, const gic_disc_state* state, const float* q, int32_t q_rows, const int32_t* q_index,
                               float scale, int accumulate, float* logits, void* stream) {
  GIC_PROPAGATE(check_match_dims(dims, "disc_match_fwd_grouped"));
  GIC_CHECK_ARG(state, "disc_match_fwd_grouped: null state");
  GIC_CHECK_ARG(q, "disc_match_fwd_grouped: null q");
  GIC_CHECK_ARG(logits, "disc_match_fwd_grouped: null logits");
  GIC_CHECK_ARG(state->ydrop, "disc_match_fwd_grouped: null state buffer (ydrop)");
  GIC_CHECK_ARG((((uintptr_t)state->ydrop) & 15) == 0, "disc_match_fwd_grouped: ydrop must be 16-byte aligned");
  GIC_CHECK_ARG(scale == scale, "disc_match_fwd_grouped: scale is NaN");
  GIC_CHECK_ARG(q_rows >= 1, "disc_match_fwd_grouped: q_rows=%d must be >= 1", q_rows);
  GIC_CHECK_ARG(q_index || q_rows == dims->B, "disc_match_fwd_grouped: q_index is NULL (the identity), so q_rows=%d must equal B=%d", q_rows,
                dims->B);
  return launch_match_fwd(dims, state->ydrop, q, q_rows, q_index, scale, accumulate, logits, (hipStream_t)stream, "disc_match_fwd_grouped");
}

int gic_gan_losses_mismatch(float w, int64_t n, float* losses_a, const float* losses_b, float* dd_real_a, float* dd_fake_a,
                            const float* dd_real_b, float* dd_fake_b, void* stream) {
  GIC_CHECK_ARG(w >= 0.f && w < 1.f, "gan_losses_mismatch: weight %g must be in [0, 1)", (double)w);
  GIC_CHECK_ARG(n >= 1 && losses_a && losses_b, "gan_losses_mismatch: null losses or n < 1");
  const bool grads = dd_real_a || dd_fake_a || dd_real_b || dd_fake_b;
  GIC_CHECK_ARG(!grads || (dd_real_a && dd_fake_a && dd_real_b && dd_fake_b), "gan_losses_mismatch: pass all four gradient vectors or none");
  hipLaunchKernelGGL(gan_losses_mix_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, w, (long)n, losses_a, losses_b, dd_real_a,
                     dd_fake_a, dd_real_b, dd_fake_b);
  GIC_CHECK_LAUNCH("gan_losses_mismatch");
  return GIC_OK;
}

}  // extern "C"
