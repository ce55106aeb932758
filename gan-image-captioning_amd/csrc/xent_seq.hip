// Masked, label-smoothed sequence cross entropy with per-caption log-likelihoods (gicap.h gic_xent_seq).
// Three launches, no f32 atomics, every sum in a fixed order:
//   xent_seq_count   one workgroup: cap_tokens[b] = the counted rows of caption b (a wave per caption, integer sums), loss[1] = count.
//   xent_seq_rows    one 256-thread workgroup per row.  An uncounted row writes zeros (row_nll, its loss term, its gradient row) and reads
//                    no logit.  A counted row reads its logits ONCE with 16-byte loads, every lane keeping a running (max, sum exp(x - max),
//                    sum (x - c), x_t) -- c = the row's first logit, so that the sum for the smoothing term carries no common offset --
//                    merges them through one LDS hop, and then reads the row a second time (an L2 hit: the row is 40 KB at V = 10 000) for
//                    the gradient p - (1 - eps) onehot - eps / V.  A row address that is not 16-byte aligned (V * sizeof % 16 != 0) takes
//                    its first elements up to the boundary and what is left after the last whole vector as scalars: no vector access is
//                    ever misaligned.  bf16 rows travel as short8.
//   xent_seq_fold    one workgroup: cap_nll[b] = the row_nll of caption b added in index order (a thread per caption), loss[0] = the
//                    rows' loss terms summed in block_sum's order / count (0 when nothing is counted).
// nll = (max - x_t) + log(sum): the log-sum-exp is never formed as one f32 number, so a common offset of the logits costs no digits.
#include "../../include/gicap.h"
#include "kernels.h"

namespace gic {
namespace {

typedef short short8 __attribute__((ext_vector_type(8)));

template <typename TA> struct RowVec;
template <> struct RowVec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float (&f)[4]) {
    const f32x4 v = *(const f32x4*)p;
    f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
  }
  static __device__ __forceinline__ void store(float* p, const float (&f)[4]) {
    f32x4 v;
    v[0] = f[0]; v[1] = f[1]; v[2] = f[2]; v[3] = f[3];
    *(f32x4*)p = v;
  }
};
template <> struct RowVec<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float (&f)[8]) {
    const short8 v = *(const short8*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = __uint_as_float((unsigned int)(unsigned short)v[k] << 16);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&f)[8]) {
    bf16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (bf16_t)f[k];
    *(bf16x8*)p = v;
  }
};

// the split of a row of V elements at address x: [0, head) scalars up to the 16-byte boundary, nvec whole vectors, the rest scalars
template <typename TA>
__device__ __forceinline__ void row_split(const TA* x, int V, int& head, int& nvec) {
  constexpr int N = RowVec<TA>::N;
  const uintptr_t a = (uintptr_t)x;
  if (a % sizeof(TA)) { head = V; nvec = 0; return; }        // not even element-aligned: no vector access at all
  const int h = (int)(((16 - (a & 15)) & 15) / sizeof(TA));
  head = h < V ? h : V;
  nvec = (V - head) / N;
}

__device__ __forceinline__ bool row_counted(long row, int group, const int32_t* lengths, const int64_t* targets, int64_t ignore_index) {
  if (targets[row] == ignore_index) return false;
  return !lengths || (int)(row % group) < lengths[row / group];
}

struct RowStat {
  float m, s, sx, xt;       // running max, sum exp(x - m), sum (x - c), the target's logit (0 until seen)
};

__device__ __forceinline__ void stat_add(RowStat& st, float x, int idx, int tgt, float c) {
  if (x > st.m) { st.s *= expf(st.m - x); st.m = x; }
  st.s += expf(x - st.m);
  st.sx += x - c;
  st.xt = idx == tgt ? x : st.xt;
}

template <int N>
__device__ __forceinline__ void stat_add_vec(RowStat& st, const float (&f)[N], int i0, int tgt, float c) {
  float vm = f[0];
#pragma unroll
  for (int k = 1; k < N; ++k) vm = fmaxf(vm, f[k]);
  if (vm > st.m) { st.s *= expf(st.m - vm); st.m = vm; }       // one rescale per vector; exp(-inf) = 0 on the first
  float e = 0.f, d = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    e += expf(f[k] - st.m);
    d += f[k] - c;
    st.xt = (i0 + k) == tgt ? f[k] : st.xt;
  }
  st.s += e;
  st.sx += d;
}

__global__ __launch_bounds__(1024) void xent_seq_count_kernel(const int64_t* __restrict__ targets, long rows, int group,
                                                               const int32_t* __restrict__ lengths, int64_t ignore_index,
                                                               int32_t* __restrict__ cap_tokens, float* __restrict__ loss) {
  __shared__ long red[16];
  const long caps = rows / group;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long total = 0;
  for (long b = w; b < caps; b += 16) {
    int n = 0;
    for (int t = lane; t < group; t += 64) n += row_counted(b * group + t, group, lengths, targets, ignore_index) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0 && cap_tokens) cap_tokens[b] = n;
    total += n;
  }
  if (lane == 0) red[w] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    long c = 0;
    for (int i = 0; i < 16; ++i) c += red[i];
    loss[1] = (float)c;
  }
}

template <typename TA>
__global__ __launch_bounds__(256) void xent_seq_rows_kernel(const TA* __restrict__ logits, int V, const int64_t* __restrict__ targets,
                                                             int group, const int32_t* __restrict__ lengths, int64_t ignore_index,
                                                             float smoothing, const float* __restrict__ row_weight,
                                                             const float* __restrict__ loss, float* __restrict__ row_nll,
                                                             float* __restrict__ row_loss, TA* __restrict__ dlogits) {
  constexpr int N = RowVec<TA>::N;
  __shared__ float red[16];
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  const TA* x = logits + row * V;
  TA* dx = dlogits ? dlogits + row * V : nullptr;
  int head, nvec;
  row_split<TA>(x, V, head, nvec);
  const int tail0 = head + nvec * N, nscal = head + (V - tail0);       // scalar element i: i < head ? i : tail0 + (i - head)
  const TA* xv = x + head;
  // the gradient row takes vector stores where it is aligned like the logits row (the same split), scalar stores otherwise
  const bool dvec = dx && (((uintptr_t)dx ^ (uintptr_t)x) & 15) == 0;

  if (!row_counted(row, group, lengths, targets, ignore_index)) {      // the same for every thread of the workgroup
    if (tid == 0) { row_nll[row] = 0.f; row_loss[row] = 0.f; }
    if (dx) {
      float z[N];
#pragma unroll
      for (int k = 0; k < N; ++k) z[k] = 0.f;
      if (dvec) {
        for (int q = tid; q < nvec; q += 256) RowVec<TA>::store(dx + head + q * N, z);
        for (int i = tid; i < nscal; i += 256) dx[i < head ? i : tail0 + (i - head)] = from_f32<TA>(0.f);
      } else {
        for (int v = tid; v < V; v += 256) dx[v] = from_f32<TA>(0.f);
      }
    }
    return;
  }

  long tgt64 = targets[row];
  // a counted target outside [0, V) poisons the loss (as gic_xent does); the index is clamped here, before anything is addressed with it
  const bool bad = tgt64 < 0 || tgt64 >= V;
  const int tgt = bad ? 0 : (int)tgt64;
  const float c = to_f32<TA>(x[0]);
  RowStat st = {-INFINITY, 0.f, 0.f, 0.f};
  for (int q = tid; q < nvec; q += 512) {                              // two 16-byte loads in flight per lane
    float a[N], b[N];
    const bool two = q + 256 < nvec;
    RowVec<TA>::load(xv + q * N, a);
    if (two) RowVec<TA>::load(xv + (q + 256) * N, b);
    stat_add_vec<N>(st, a, head + q * N, tgt, c);
    if (two) stat_add_vec<N>(st, b, head + (q + 256) * N, tgt, c);
  }
  for (int i = tid; i < nscal; i += 256) {
    const int v = i < head ? i : tail0 + (i - head);
    stat_add(st, to_f32<TA>(x[v]), v, tgt, c);
  }
  const float mx = block_max(st.m, red);
  const float s = block_sum(st.s * expf(st.m - mx), red);               // a lane that saw nothing: 0 * exp(-inf) = 0
  const float sx = block_sum(st.sx, red);
  const float xt = block_sum(st.xt, red);                              // one lane holds it, the others add zeros
  const float logs = logf(s);
  const float nll = (mx - xt) + logs;
  const float wgt = row_weight ? row_weight[row] : 1.f;
  if (tid == 0) {
    const float uni = ((mx - c) - sx / (float)V) + logs;               // -mean_v log p_v
    row_nll[row] = bad ? NAN : nll;
    row_loss[row] = bad ? NAN : wgt * ((1.f - smoothing) * nll + smoothing * uni);
  }
  if (!dx) return;

  const float scale = wgt / loss[1];                                   // count >= 1: this row is counted
  const float inv_s = 1.f / s;
  const float hit = 1.f - smoothing, uni = smoothing / (float)V;
  auto grad = [&](float xv_, int v) { return (expf(xv_ - mx) * inv_s - (v == tgt ? hit : 0.f) - uni) * scale; };
  for (int q = tid; q < nvec; q += 512) {
    float a[N], b[N];
    const bool two = q + 256 < nvec;
    RowVec<TA>::load(xv + q * N, a);
    if (two) RowVec<TA>::load(xv + (q + 256) * N, b);
    const int ia = head + q * N, ib = head + (q + 256) * N;
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = grad(a[k], ia + k);
    if (dvec) {
      RowVec<TA>::store(dx + ia, a);
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) dx[ia + k] = from_f32<TA>(a[k]);
    }
    if (two) {
#pragma unroll
      for (int k = 0; k < N; ++k) b[k] = grad(b[k], ib + k);
      if (dvec) {
        RowVec<TA>::store(dx + ib, b);
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k) dx[ib + k] = from_f32<TA>(b[k]);
      }
    }
  }
  for (int i = tid; i < nscal; i += 256) {
    const int v = i < head ? i : tail0 + (i - head);
    dx[v] = from_f32<TA>(grad(to_f32<TA>(x[v]), v));
  }
}

__global__ __launch_bounds__(1024) void xent_seq_fold_kernel(const float* __restrict__ row_nll, const float* __restrict__ row_loss, long rows,
                                                              int group, float* __restrict__ cap_nll, float* __restrict__ loss) {
  __shared__ float red[16];
  if (cap_nll) {
    const long caps = rows / group;
    for (long b = threadIdx.x; b < caps; b += 1024) {
      float s = 0.f;
      for (int t = 0; t < group; ++t) s += row_nll[b * group + t];
      cap_nll[b] = s;
    }
  }
  float s = 0.f;
  for (long i = threadIdx.x; i < rows; i += 1024) s += row_loss[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const float count = loss[1];
    loss[0] = count > 0.f ? s / count : 0.f;
  }
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" int gic_xent_seq(const void* logits, int dtype, int64_t rows, int32_t V, const int64_t* targets, int64_t group,
                            const int32_t* lengths, int64_t ignore_index, float smoothing, const float* row_weight, float* loss,
                            float* row_nll, float* row_ws, float* cap_nll, int32_t* cap_tokens, void* d_logits, void* stream_) {
  GIC_CHECK_ARG(logits, "xent_seq: null logits");
  GIC_CHECK_ARG(targets, "xent_seq: null targets");
  GIC_CHECK_ARG(loss, "xent_seq: null loss");
  GIC_CHECK_ARG(row_nll, "xent_seq: null row_nll");
  GIC_CHECK_ARG(row_ws, "xent_seq: null row_ws");
  GIC_CHECK_ARG(rows > 0, "xent_seq: rows=%lld must be positive", (long long)rows);
  // one 256-thread workgroup per row: a grid carries fewer than 2^32 threads, and the count in loss[1] is exact as f32 up to 2^24
  GIC_CHECK_ARG(rows < (1LL << 24), "xent_seq: rows=%lld exceeds 2^24 - 1 (a 256-thread workgroup per row; the f32 count)", (long long)rows);
  GIC_CHECK_ARG(V > 0, "xent_seq: V=%d must be positive", V);
  GIC_CHECK_ARG(group >= 1 && group <= 0x7fffffffLL, "xent_seq: group=%lld must be at least 1", (long long)group);
  GIC_CHECK_ARG(rows % group == 0, "xent_seq: group=%lld does not divide rows=%lld", (long long)group, (long long)rows);
  GIC_CHECK_ARG(smoothing >= 0.f && smoothing < 1.f, "xent_seq: smoothing=%g must be in [0, 1)", (double)smoothing);      // false for NaN
  if (dtype != DT_F32 && dtype != DT_BF16) { set_last_error("xent_seq: bad dtype %d", dtype); return GIC_ERR_UNSUPPORTED; }
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(xent_seq_count_kernel, dim3(1), dim3(1024), 0, stream, targets, (long)rows, (int)group, lengths, ignore_index, cap_tokens,
                     loss);
  GIC_CHECK_LAUNCH("xent_seq_count");
  if (dtype == DT_F32)
    hipLaunchKernelGGL((xent_seq_rows_kernel<float>), dim3((unsigned)rows), dim3(256), 0, stream, (const float*)logits, V, targets, (int)group,
                       lengths, ignore_index, smoothing, row_weight, (const float*)loss, row_nll, row_ws, (float*)d_logits);
  else
    hipLaunchKernelGGL((xent_seq_rows_kernel<bf16_t>), dim3((unsigned)rows), dim3(256), 0, stream, (const bf16_t*)logits, V, targets, (int)group,
                       lengths, ignore_index, smoothing, row_weight, (const float*)loss, row_nll, row_ws, (bf16_t*)d_logits);
  GIC_CHECK_LAUNCH("xent_seq_rows");
  hipLaunchKernelGGL(xent_seq_fold_kernel, dim3(1), dim3(1024), 0, stream, (const float*)row_nll, (const float*)row_ws, (long)rows, (int)group,
                     cap_nll, loss);
  GIC_CHECK_LAUNCH("xent_seq_fold");
  return GIC_OK;
}
