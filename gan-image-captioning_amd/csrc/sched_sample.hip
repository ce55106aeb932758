// Scheduled sampling for the teacher-forced decodes (gicap.h gic_decoder_forward_ss / gic_attn_forward_ss; Bengio et al., 2015): the
// input of step t is the ground truth with probability 1 - p, else a token picked from the model's own logits of step t-1.  The choice
// sits on the recurrence's serial chain (logits of t-1 -> coin -> pick -> embedding row -> gate product of t), so one launch does all of
// it between two steps:
//   ss_pick   one 256-thread workgroup per caption.  Not replaced (coin >= p, or t >= lengths[b]): the workgroup writes inputs / replaced
//             and returns without reading a logit -- the teacher's embedding row is in place since embed_rows_tf.  Replaced: the argmax
//             of l[v] (+ Gumbel(u[v])) over the vocabulary as the maximum of row_key() keys -- (value, lowest index) order, integer
//             compares only, so the order of the lanes and waves does not matter; 16-byte loads of the logits and the uniforms where
//             V % 4 == 0 (rows 16-byte aligned), scalar otherwise -- then the pick's embedding row into x of slot t.
//   ss_tail   positions >= Tmax - 1 of inputs (never fed): copies of caps, replaced = 0.
// The coin and the uniforms come from the caller's buffers or from Philox keyed by (seed, stream tag | t, caption): a caption's draws do
// not depend on the batch it sits in.  No f32 atomics: the same inputs give the same bits.
#include "../../include/gicap.h"
#include "decoder_step.h"
#include "kernels.h"

namespace gic {
namespace {

constexpr uint64_t kSsCoinStream = (uint64_t)0x7373636f << 32;    // "ssco" | t
constexpr uint64_t kSsNoiseStream = (uint64_t)0x73736e6f << 32;   // "ssno" | t

__device__ __forceinline__ float ss_gumbel(float u) {
  const float eps = 1e-10f;
  return -logf(-logf(u + eps) + eps);
}

__device__ __forceinline__ unsigned long long ss_wave_max(unsigned long long k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned int hi = __shfl_xor((unsigned int)(k >> 32), o, 64), lo = __shfl_xor((unsigned int)k, o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    k = other > k ? other : k;
  }
  return k;
}

template <typename TA>
__global__ __launch_bounds__(256) void ss_pick_kernel(const SsPickArgs a) {
  __shared__ unsigned long long red[4];
  const int b = blockIdx.x, tid = threadIdx.x, V = a.V;
  const long pos = (long)b * a.Tm1 + (a.t - 1);
  float coin;
  if (a.coin_u) {
    coin = a.coin_u[pos];
  } else {
    uint32_t r0, r1, r2, r3;
    Philox::gen4(a.seed, kSsCoinStream | (uint64_t)a.t, (uint64_t)b, r0, r1, r2, r3);
    coin = Philox::u01(r0);
  }
  if (!(coin < a.prob && a.t < a.lengths[b])) {           // the same for every thread of the workgroup
    if (tid == 0) {
      const long id = a.caps[pos];
      a.inputs[pos] = id < 0 ? 0 : (id >= V ? V - 1 : id);
      if (a.replaced) a.replaced[pos] = 0;
    }
    return;
  }
  const float* row = a.logits + (long)b * a.ld_logits;
  const bool noisy = a.pick == 0;
  const float* urow = noisy && a.noise_u ? a.noise_u + ((long)(a.t - 1) * a.B + b) * V : nullptr;
  const uint64_t nstream = kSsNoiseStream | (uint64_t)a.t, nbase = (uint64_t)b << 32;
  unsigned long long best = 0;                             // below every key
  const bool vec = V % 4 == 0 && ((uintptr_t)row & 15) == 0 && ((uintptr_t)urow & 15) == 0;
  const int nq = vec ? V / 4 : 0;
  for (int q = tid; q < nq; q += 256) {
    const f32x4 l = *(const f32x4*)(row + 4 * q);
    float y[4] = {l[0], l[1], l[2], l[3]};
    if (noisy) {
      float u[4];
      if (urow) {
        const f32x4 uu = *(const f32x4*)(urow + 4 * q);
        u[0] = uu[0]; u[1] = uu[1]; u[2] = uu[2]; u[3] = uu[3];
      } else {
        uint32_t r0, r1, r2, r3;
        Philox::gen4(a.seed, nstream, nbase | (uint64_t)q, r0, r1, r2, r3);
        u[0] = Philox::u01(r0); u[1] = Philox::u01(r1); u[2] = Philox::u01(r2); u[3] = Philox::u01(r3);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] += ss_gumbel(u[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned long long k = row_key(y[i], 4 * q + i);
      best = k > best ? k : best;
    }
  }
  for (int v = 4 * nq + tid; v < V; v += 256) {            // the whole row when it takes no 16-byte loads
    float y = row[v];
    if (noisy) {
      float u;
      if (urow) {
        u = urow[v];
      } else {
        uint32_t r[4];
        Philox::gen(a.seed, nstream, nbase | (uint64_t)(v >> 2), r);
        u = Philox::u01(r[v & 3]);
      }
      y += ss_gumbel(u);
    }
    const unsigned long long k = row_key(y, v);
    best = k > best ? k : best;
  }
  best = ss_wave_max(best);
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  best = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) best = red[w] > best ? red[w] : best;
  int id = row_key_index(best);
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);                // every key carries an index in [0, V): a guard, not a path
  if (tid == 0) {
    a.inputs[pos] = id;
    if (a.replaced) a.replaced[pos] = 1;
  }
  TA* x = (TA*)a.x_next + (long)b * a.ld_x;
  for (int e = tid; e < a.E; e += 256) x[e] = from_f32<TA>(a.embed[(long)id * a.E + e]);
}

__global__ void ss_tail_kernel(const int64_t* __restrict__ caps, int64_t* __restrict__ inputs, int32_t* __restrict__ replaced, int B,
                               int Tm1, int from) {
  const int w = Tm1 - from;
  const long total = (long)B * w;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long pos = (i / w) * Tm1 + from + (i % w);
    inputs[pos] = caps[pos];
    if (replaced) replaced[pos] = 0;
  }
}

}  // namespace

int ss_check_opts(const gic_sched_sample_opts* o, int L, const char* what) {
  GIC_CHECK_ARG(o, "%s: null opts", what);
  GIC_CHECK_ARG(o->prob >= 0.f && o->prob <= 1.f, "%s: prob must be in [0, 1]", what);      // false for NaN
  GIC_CHECK_ARG(o->pick == 0 || o->pick == 1, "%s: pick must be 0 (sample) or 1 (argmax)", what);
  GIC_CHECK_ARG(L == 1 || o->inputs, "%s: opts->inputs is null", what);      // L = 1: no position to decide
  return GIC_OK;
}

int ss_pick(const SsPickArgs& a, int dt, hipStream_t stream) {
  GIC_CHECK_ARG(a.logits && a.caps && a.lengths && a.embed && a.x_next && a.inputs, "ss_pick: null buffer");
  GIC_CHECK_ARG(a.B > 0 && a.V > 0 && a.E > 0 && a.t >= 1 && a.t <= a.Tm1, "ss_pick: bad dims");
  if (dt == DT_F32) hipLaunchKernelGGL((ss_pick_kernel<float>), dim3((unsigned)a.B), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((ss_pick_kernel<bf16_t>), dim3((unsigned)a.B), dim3(256), 0, stream, a);
  GIC_CHECK_LAUNCH("ss_pick");
  return GIC_OK;
}

int ss_tail(const int64_t* caps, int64_t* inputs, int32_t* replaced, int B, int Tm1, int from, hipStream_t stream) {
  if (from >= Tm1) return GIC_OK;
  const long total = (long)B * (Tm1 - from);
  hipLaunchKernelGGL(ss_tail_kernel, dim3((unsigned)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256)), dim3(256), 0, stream, caps,
                     inputs, replaced, B, Tm1, from);
  GIC_CHECK_LAUNCH("ss_tail");
  return GIC_OK;
}

int ss_step_logits(int dt, const void* hout, int t, int Tmax, const void* wout, const float* b_out, float* logits, int B, int V, int H,
                   bool fused, hipStream_t stream) {
  const void* h = (const char*)hout + (size_t)t * H * dtype_size(dt);
  if (fused) {
    VocabStepArgs v;
    v.h = h; v.ldh = (long)Tmax * H; v.wout = wout; v.bias = b_out;
    v.logits = logits + (long)t * V; v.ld_logits = (long)Tmax * V;
    v.B = B; v.V = V; v.H = H;
    return vocab_step_logits(v, dt, stream);
  }
  GemmDesc g;
  g.A = h; g.lda = (long)Tmax * H; g.B = wout; g.ldb = H; g.C = logits + (long)t * V; g.ldc = (long)Tmax * V;
  g.M = B; g.N = V; g.K = H; g.in_dtype = dt; g.out_dtype = DT_F32; g.bias = b_out;
  g.no_split = 1;
  return gemm(g, stream);
}

}  // namespace gic
