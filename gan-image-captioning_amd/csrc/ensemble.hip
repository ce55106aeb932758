// Ensemble mixing of per-member logits (gicap.h gic_ensemble_mix; the mixing step of decode.hip's ensemble searches).
//   logits f32 [M][rows][V] (member stride given)  ->  z f32 [rows][V]
//   lp_m = l_m - logsumexp(l_m) per row
//   prob     z[v] = log sum_m w_m exp(lp_m[v])      as a + log sum_m exp(t_m - a), t_m = (log w_m - lse_m) + l_m[v], a = max_m t_m
//   logprob  z[v] = sum_m w_m lp_m[v]               m = 0..M-1 in order
// One row per workgroup of 4 waves (V > kWaveRowV), else one row per wave.  Pass 1 (row_lse): every lane keeps M online
// (max, sum-exp) pairs over its 16-byte vectors (vector i of the row to lane i % T, T = the row's lanes) and, the lanes below V % 4, one
// tail column each; the pairs are merged across the wave by an xor butterfly and across the row's waves through LDS in wave order, by
// every lane alike.  Pass 2 re-reads the row (from L2: the row was just read) and writes z (mix_one per element).  Every exp has its
// maximum subtracted first, so logits of magnitude 1e4 stay finite; a member whose term underflows adds 0 (prob) and its true
// log-probability (logprob).  No atomics and a fixed order: the same bits on every call.  Rows of a V that is no multiple of 4 are not
// 16-byte aligned: the vector type below carries 4-byte alignment, which global memory accesses of gfx9 take in hardware.
#include <math.h>

#include <cfloat>

#include "../../include/gicap.h"
#include "beam.h"

namespace gic {
namespace {

constexpr int kMixThreads = 256;
constexpr int kMixWaves = kMixThreads / WAVE;
constexpr int kWaveRowV = 1024;          // up to here a row is one wave's (4 trips of 16-byte vectors at the most)

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

struct MixWeights { float w[GIC_MAX_ENSEMBLE]; float logw[GIC_MAX_ENSEMBLE]; };

// (m, s) <- (m, s) + (m2, s2): sum-exp pairs at their own maxima; a pair that holds nothing is (-inf, 0)
__device__ __forceinline__ void pair_merge(float& m, float& s, float m2, float s2) {
  const float n = fmaxf(m, m2);
  s = (m == n ? s : s * expf(m - n)) + (m2 == n ? s2 : s2 * expf(m2 - n));
  m = n;
}

// Pass 1 of one row (base: member 0's row; member m at base + m * mstride) by the T = WPR * 64 lanes that hold it, lane = 0..T-1:
// lse[m] = logsumexp of member m's row, in every lane.  red_m / red_s: LDS [kMixWaves][GIC_MAX_ENSEMBLE], used with WPR > 1 only (then
// every thread of the workgroup must call)
template <int M, int WPR>
__device__ __forceinline__ void row_lse(const float* __restrict__ base, long mstride, int V, int lane, float (&lse)[M],
                                        float (*red_m)[GIC_MAX_ENSEMBLE], float (*red_s)[GIC_MAX_ENSEMBLE]) {
  constexpr int T = WPR * WAVE;
  const int nvec = V >> 2, tail = V & 3;
  float mx[M], sm[M];
#pragma unroll
  for (int m = 0; m < M; ++m) { mx[m] = -INFINITY; sm[m] = 0.f; }
  for (int i = lane; i < nvec; i += T) {
    f32x4u x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = *(const f32x4u*)(base + m * mstride + 4 * i);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float n = fmaxf(fmaxf(fmaxf(x[m].x, x[m].y), fmaxf(x[m].z, x[m].w)), mx[m]);
      const float e = ((expf(x[m].x - n) + expf(x[m].y - n)) + expf(x[m].z - n)) + expf(x[m].w - n);
      sm[m] = (mx[m] == n ? sm[m] : sm[m] * expf(mx[m] - n)) + e;
      mx[m] = n;
    }
  }
  if (lane < tail) {
#pragma unroll
    for (int m = 0; m < M; ++m) pair_merge(mx[m], sm[m], base[m * mstride + 4 * nvec + lane], 1.f);
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) pair_merge(mx[m], sm[m], __shfl_xor(mx[m], o, WAVE), __shfl_xor(sm[m], o, WAVE));
  }
  if constexpr (WPR > 1) {
    const int tid = threadIdx.x;
    if ((tid & (WAVE - 1)) == 0) {
#pragma unroll
      for (int m = 0; m < M; ++m) { red_m[tid / WAVE][m] = mx[m]; red_s[tid / WAVE][m] = sm[m]; }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m) {
      mx[m] = red_m[0][m]; sm[m] = red_s[0][m];
#pragma unroll
      for (int w = 1; w < WPR; ++w) pair_merge(mx[m], sm[m], red_m[w][m], red_s[w][m]);
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) lse[m] = mx[m] + logf(sm[m]);
}

// the members' constants of pass 2: prob  c_m = log w_m - lse_m; logprob  c_m = lse_m
template <int M>
__device__ __forceinline__ void mix_consts(int mode, const MixWeights& wt, const float (&lse)[M], float (&c)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) c[m] = mode == GIC_ENSEMBLE_PROB ? wt.logw[m] - lse[m] : lse[m];
}

// z of one element from the members' logits l[0..M)
template <int M>
__device__ __forceinline__ float mix_one(int mode, const MixWeights& wt, const float (&c)[M], const float (&l)[M]) {
  if (mode == GIC_ENSEMBLE_PROB) {
    float t[M], a = -INFINITY;
#pragma unroll
    for (int m = 0; m < M; ++m) { t[m] = c[m] + l[m]; a = fmaxf(a, t[m]); }
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) s += expf(t[m] - a);
    return a + logf(s);
  }
  float z = 0.f;
#pragma unroll
  for (int m = 0; m < M; ++m) z += wt.w[m] * (l[m] - c[m]);
  return z;
}

template <int M, int MODE, int WPR>      // WPR: waves per row (4: a workgroup per row, 1: a wave per row)
__global__ __launch_bounds__(kMixThreads) void ensemble_mix_kernel(const float* __restrict__ logits, long mstride, int rows, int V,
                                                                   const MixWeights wt, float* __restrict__ out, const int* stop,
                                                                   int stop_at) {
  if (stop && *stop >= stop_at) return;
  constexpr int T = WPR * WAVE, RPB = kMixThreads / T;
  __shared__ float red_m[kMixWaves][GIC_MAX_ENSEMBLE], red_s[kMixWaves][GIC_MAX_ENSEMBLE];
  const int tid = threadIdx.x, lane = tid % T;
  const long row = (long)blockIdx.x * RPB + tid / T;
  const bool live = row < rows;          // (a whole wave at WPR = 1; every row is live at WPR = 4)
  const float* base = logits + (live ? row : 0) * V;
  const int nvec = V >> 2, tail = V & 3;
  float lse[M], c[M];
  row_lse<M, WPR>(base, mstride, V, lane, lse, red_m, red_s);
  if (!live) return;
  mix_consts<M>(MODE, wt, lse, c);

  float* orow = out + row * V;
  for (int i = lane; i < nvec; i += T) {
    f32x4u x[M], z;
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = *(const f32x4u*)(base + m * mstride + 4 * i);
    float l[M];
#pragma unroll
    for (int m = 0; m < M; ++m) l[m] = x[m].x;
    z.x = mix_one<M>(MODE, wt, c, l);
#pragma unroll
    for (int m = 0; m < M; ++m) l[m] = x[m].y;
    z.y = mix_one<M>(MODE, wt, c, l);
#pragma unroll
    for (int m = 0; m < M; ++m) l[m] = x[m].z;
    z.z = mix_one<M>(MODE, wt, c, l);
#pragma unroll
    for (int m = 0; m < M; ++m) l[m] = x[m].w;
    z.w = mix_one<M>(MODE, wt, c, l);
    *(f32x4u*)(orow + 4 * i) = z;
  }
  if (lane < tail) {
    float l[M];
#pragma unroll
    for (int m = 0; m < M; ++m) l[m] = base[m * mstride + 4 * nvec + lane];
    orow[4 * nvec + lane] = mix_one<M>(MODE, wt, c, l);
  }
}

template <int M, int MODE>
int launch_mix(const float* logits, long mstride, int rows, int V, const MixWeights& wt, float* out, const int* stop, int stop_at,
               hipStream_t stream) {
  if (V > kWaveRowV)
    hipLaunchKernelGGL((ensemble_mix_kernel<M, MODE, 4>), dim3((unsigned)rows), dim3(kMixThreads), 0, stream, logits, mstride, rows, V, wt, out,
                       stop, stop_at);
  else
    hipLaunchKernelGGL((ensemble_mix_kernel<M, MODE, 1>), dim3((unsigned)cdiv(rows, kMixWaves)), dim3(kMixThreads), 0, stream, logits,
                       mstride, rows, V, wt, out, stop, stop_at);
  GIC_CHECK_LAUNCH("ensemble_mix");
  return GIC_OK;
}

template <int M>
int launch_mix_mode(int mode, const float* logits, long mstride, int rows, int V, const MixWeights& wt, float* out, const int* stop, int stop_at,
                    hipStream_t stream) {
  if (mode == GIC_ENSEMBLE_PROB) return launch_mix<M, GIC_ENSEMBLE_PROB>(logits, mstride, rows, V, wt, out, stop, stop_at, stream);
  return launch_mix<M, GIC_ENSEMBLE_LOGPROB>(logits, mstride, rows, V, wt, out, stop, stop_at, stream);
}

// the weights as the kernels take them: normalised in double, w and log w rounded to f32
MixWeights mix_weights(const gic_ensemble_opts& o) {
  MixWeights wt{};
  double sum = 0.0;
  for (int m = 0; m < o.M; ++m) sum += (double)o.weights[m];
  for (int m = 0; m < o.M; ++m) {
    const double w = (double)o.weights[m] / sum;
    wt.w[m] = (float)w;
    wt.logw[m] = (float)log(w);
  }
  return wt;
}

}  // namespace

int check_ensemble_opts(const gic_ensemble_opts* o, const char* who) {
  GIC_CHECK_ARG(o, "%s: null ensemble options", who);
  GIC_CHECK_ARG(o->M >= 1 && o->M <= GIC_MAX_ENSEMBLE, "%s: M must be 1..%d, got %d", who, GIC_MAX_ENSEMBLE, o->M);
  GIC_CHECK_ARG(o->mode == GIC_ENSEMBLE_PROB || o->mode == GIC_ENSEMBLE_LOGPROB, "%s: mode must be 0 (prob) or 1 (logprob), got %d", who,
                o->mode);
  for (int m = 0; m < o->M; ++m)
    GIC_CHECK_ARG(o->weights[m] > 0.f && o->weights[m] <= FLT_MAX, "%s: weights[%d] must be finite and > 0", who, m);
  return GIC_OK;
}

int ensemble_mix(const float* logits, long mstride, int rows, int V, const gic_ensemble_opts& o, float* out, const int* stop, int stop_at,
                 hipStream_t stream) {
  const MixWeights wt = mix_weights(o);
  switch (o.M) {
    case 1: return launch_mix_mode<1>(o.mode, logits, mstride, rows, V, wt, out, stop, stop_at, stream);
    case 2: return launch_mix_mode<2>(o.mode, logits, mstride, rows, V, wt, out, stop, stop_at, stream);
    case 3: return launch_mix_mode<3>(o.mode, logits, mstride, rows, V, wt, out, stop, stop_at, stream);
    default: return launch_mix_mode<4>(o.mode, logits, mstride, rows, V, wt, out, stop, stop_at, stream);
  }
}

}  // namespace gic

using namespace gic;

extern "C" int gic_ensemble_mix(const float* logits, int32_t M, int64_t rows, int32_t V, const float* weights, int32_t mode, float* out,
                                void* stream) {
  GIC_CHECK_ARG(M >= 1 && M <= GIC_MAX_ENSEMBLE, "ensemble_mix: M must be 1..%d, got %d", GIC_MAX_ENSEMBLE, M);
  GIC_CHECK_ARG(rows >= 1 && rows <= (1l << 24) && V >= 2, "ensemble_mix: rows must be 1..2^24 and V >= 2");
  GIC_CHECK_ARG(logits && weights && out, "ensemble_mix: null argument");
  GIC_CHECK_ARG((((uintptr_t)logits | (uintptr_t)out) & 3) == 0, "ensemble_mix: logits and out must be 4-byte aligned");
  gic_ensemble_opts o{};
  o.M = M; o.mode = mode;
  for (int m = 0; m < M; ++m) o.weights[m] = weights[m];
  GIC_PROPAGATE(check_ensemble_opts(&o, "ensemble_mix"));
  return ensemble_mix(logits, (long)rows * V, (int)rows, V, o, out, nullptr, 0, (hipStream_t)stream);
}
