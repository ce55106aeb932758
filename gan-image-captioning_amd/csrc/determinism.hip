// Deterministic mode (gic_set_deterministic): the process-wide switch and the fixed-order reductions that replace f32 atomics
// whose adders race.  Every f32 sum that more than one workgroup contributes to gets a fixed order here:
//   - det_scatter: embedding-gradient scatters.  The token positions are sorted by (id, position) in LDS, then each (id, column)
//     is summed by ONE lane in ascending position order (long runs: 16 waves over fixed sub-ranges, folded in wave order);
//   - bn_stats: BatchNorm column sums of a trunk convolution's output ([rows, C], NHWC), per-part partials with plain stores into a
//     [P][2][C] slab, then one fold over the parts in index order into replica 0 of the layer's statistics.
// The other sites (split-K, column sums, D's weight gradients) keep their kernels and change their launch in this mode.
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "kernels.h"

namespace gic {

namespace {

std::atomic<int> g_det{[] {
  const char* e = getenv("GIC_DETERMINISTIC");
  return (e && e[0] && strcmp(e, "0") != 0) ? 1 : 0;
}()};

// ---- scatter: ids are clamped to [0, V); key = id << 13 | position (n <= 8192, V <= 2^19): unique, so the bitonic sort is stable
constexpr int kScatterMaxN = 8192;
constexpr int kScatterNT = 1024;
constexpr int kLongRun = 64;            // runs longer than this are summed by all 16 waves

// source row of token r: src[(r + row_off) * ld + e]; its id: ids[(r % B) * s_b + (r / B) * s_t]
// destination: dst[id * d_id + e * d_e] += sum
__global__ __launch_bounds__(kScatterNT) void det_scatter_kernel(const void* __restrict__ src, int dt, long ld, long row_off,
                                                                   const int64_t* __restrict__ ids, int B, long s_b, long s_t, int n,
                                                                   float* __restrict__ dst, long d_id, long d_e, int E, int V, int P) {
  __shared__ uint32_t key[kScatterMaxN];
  __shared__ int longs[kScatterMaxN / kLongRun + 1][2];
  __shared__ int nlong;
  __shared__ float red[16][64];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  for (int i = tid; i < P; i += kScatterNT) {
    uint32_t k = 0xffffffffu;
    if (i < n) {
      long id = ids[(long)(i % B) * s_b + (long)(i / B) * s_t];
      id = id < 0 ? 0 : (id >= V ? V - 1 : id);
      k = ((uint32_t)id << 13) | (uint32_t)i;
    }
    key[i] = k;
  }
  if (tid == 0) nlong = 0;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < P / 2; t += kScatterNT) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint32_t a = key[lo], b = key[hi];
        if ((a > b) == up) { key[lo] = b; key[hi] = a; }
      }
      __syncthreads();
    }
  }
  const int e = blockIdx.x * 64 + lane;
  const bool ok = e < E;
  auto load = [&](int j) -> float {
    const long r = (long)(key[j] & 8191u);
    return ok ? ld_as_f32(src, (r + row_off) * ld + e, dt) : 0.f;
  };
  auto id_of = [&](int j) -> uint32_t { return key[j] >> 13; };
  // short runs: one wave per run, the lane of column e sums the run in ascending position order
  for (int i = w; i < n; i += 16) {
    if (i > 0 && id_of(i) == id_of(i - 1)) continue;        // (wave-uniform: every lane reads the same key)
    int end = i + 1;
    while (end < n && id_of(end) == id_of(i)) ++end;
    if (end - i > kLongRun) {
      if (lane == 0) {                                       // (order of this list is free: each run is written by one pass below)
        const int q = atomicAdd(&nlong, 1);
        longs[q][0] = i; longs[q][1] = end;
      }
      continue;
    }
    float s = 0.f;
    int j = i;
    for (; j + 4 <= end; j += 4) {
      const float a0 = load(j), a1 = load(j + 1), a2 = load(j + 2), a3 = load(j + 3);
      s += a0; s += a1; s += a2; s += a3;
    }
    for (; j < end; ++j) s += load(j);
    if (ok) dst[(long)id_of(i) * d_id + (long)e * d_e] += s;
  }
  __syncthreads();
  // long runs: wave w sums the fixed sub-range w of the run, then the 16 partials fold in wave order
  const int nl = nlong;
  for (int q = 0; q < nl; ++q) {
    const int i = longs[q][0], end = longs[q][1];
    const int len = end - i, per = (len + 15) / 16;
    const int a = i + w * per, b = min(end, a + per);
    float s = 0.f;
    int j = a;
    for (; j + 4 <= b; j += 4) {
      const float a0 = load(j), a1 = load(j + 1), a2 = load(j + 2), a3 = load(j + 3);
      s += a0; s += a1; s += a2; s += a3;
    }
    for (; j < b; ++j) s += load(j);
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && ok) {
      float t = 0.f;
#pragma unroll
      for (int u = 0; u < 16; ++u) t += red[u][lane];
      dst[(long)id_of(i) * d_id + (long)e * d_e] += t;
    }
    __syncthreads();
  }
}

// ---- BatchNorm column sums: block (x, p) sums rows [p*R, (p+1)*R) of 8*CG columns; partials (sum, sum of squares) -> slab[p][2][C]
constexpr int kStatsMaxParts = 256;

template <typename T>
__global__ __launch_bounds__(256) void bn_stats_part_kernel(const T* __restrict__ y, long M, int C, int CG, long R,
                                                              float* __restrict__ slab) {
  __shared__ float red[256][17];
  const int tid = threadIdx.x, cg = tid % CG, rl = tid / CG, RL = 256 / CG;
  const int c0 = (blockIdx.x * CG + cg) * 8;
  const long r0 = (long)blockIdx.y * R, r1 = min(M, r0 + R);
  float s[8], q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = q[k] = 0.f;
  if (c0 < C && rl < RL) {
    for (long r = r0 + rl; r < r1; r += RL) {
      const T* p = y + r * C + c0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = to_f32<T>(p[k]);
        s[k] += v; q[k] += v * v;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) { red[tid][k] = s[k]; red[tid][8 + k] = q[k]; }
  __syncthreads();
  if (tid < CG * 8) {                                   // column tid of the block: fold the row lanes in order
    const int g = tid / 8, k = tid % 8, c = (blockIdx.x * CG + g) * 8 + k;
    float a = 0.f, b = 0.f;
    for (int u = 0; u < RL; ++u) { a += red[u * CG + g][k]; b += red[u * CG + g][8 + k]; }
    if (c < C) {
      slab[(long)blockIdx.y * 2 * C + c] = a;
      slab[(long)blockIdx.y * 2 * C + C + c] = b;
    }
  }
}

// stats[j] = sum over parts p (in index order) of slab[p][j], j < 2C: 64 entries x 16 part groups, folded in group order
__global__ __launch_bounds__(1024) void bn_stats_fold_kernel(const float* __restrict__ slab, int P, int C2, float* __restrict__ stats) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int per = (P + 15) / 16, a = g * per, b = min(P, a + per);
  float s = 0.f;
  if (j < C2)
    for (int p = a; p < b; ++p) s += slab[(long)p * C2 + j];
  red[g][lane] = s;
  __syncthreads();
  if (g == 0 && j < C2) {
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) t += red[u][lane];
    stats[j] = t;
  }
}

int stats_parts(long M, int C, int* CG, long* R) {
  const int groups = C / 8;
  *CG = groups < 32 ? groups : 32;
  const int gx = cdiv(groups, *CG);
  long P = 2048 / gx;
  if (P > kStatsMaxParts) P = kStatsMaxParts;
  if (P > cdiv(M, 64)) P = cdiv(M, 64);
  if (P < 1) P = 1;
  *R = (M + P - 1) / P;
  return (int)cdiv(M, *R);
}

}  // namespace

int det_mode() { return g_det.load(std::memory_order_relaxed); }

int det_scatter(const void* src, int dt, long ld, long row_off, const int64_t* ids, int B, long s_b, long s_t, long n, float* dst,
                long d_id, long d_e, int E, int V, hipStream_t stream) {
  GIC_CHECK_ARG(src && ids && dst && B > 0, "det_scatter: bad argument");
  if (n <= 0 || E <= 0) return GIC_OK;
  if (n > kScatterMaxN || V > (1 << 19)) {
    set_last_error("deterministic mode: the ordered embedding scatter takes n <= %d tokens and V <= %d (got n = %ld, V = %d)",
                   kScatterMaxN, 1 << 19, n, V);
    return GIC_ERR_UNSUPPORTED;
  }
  int P = 2;
  while (P < n) P <<= 1;
  hipLaunchKernelGGL(det_scatter_kernel, dim3((unsigned)cdiv(E, 64)), dim3(kScatterNT), 0, stream, src, dt, ld, row_off, ids, B, s_b, s_t,
                     (int)n, dst, d_id, d_e, E, V, P);
  GIC_CHECK_LAUNCH("det_scatter");
  return GIC_OK;
}

}  // namespace gic

using namespace gic;

extern "C" {

int gic_set_deterministic(int on) {
  g_det.store(on ? 1 : 0, std::memory_order_relaxed);
  return GIC_OK;
}

int gic_get_deterministic(void) { return det_mode(); }

int gic_bn_stats_slab_floats(int64_t rows, int32_t C, int64_t* out) {
  GIC_CHECK_ARG(out && rows > 0 && C > 0 && C % 8 == 0, "bn_stats_slab_floats: bad argument");
  int CG;
  long R;
  *out = (int64_t)stats_parts(rows, C, &CG, &R) * 2 * C;
  return GIC_OK;
}

int gic_bn_stats(const void* y, int dtype, int64_t rows, int32_t C, float* slab, float* stats, void* stream_) {
  GIC_CHECK_ARG(y && slab && stats && rows > 0 && C > 0, "bn_stats: bad argument");
  GIC_CHECK_ARG(C % 8 == 0, "bn_stats: C = %d is not a multiple of 8", C);
  hipStream_t stream = (hipStream_t)stream_;
  int CG;
  long R;
  const int P = stats_parts(rows, C, &CG, &R);
  const dim3 grid((unsigned)cdiv(C / 8, CG), (unsigned)P);
  if (dtype == DT_F32)
    hipLaunchKernelGGL((bn_stats_part_kernel<float>), grid, dim3(256), 0, stream, (const float*)y, (long)rows, C, CG, R, slab);
  else
    hipLaunchKernelGGL((bn_stats_part_kernel<bf16_t>), grid, dim3(256), 0, stream, (const bf16_t*)y, (long)rows, C, CG, R, slab);
  GIC_CHECK_LAUNCH("bn_stats_part");
  hipLaunchKernelGGL(bn_stats_fold_kernel, dim3((unsigned)cdiv(2 * C, 64)), dim3(1024), 0, stream, (const float*)slab, P, 2 * C, stats);
  GIC_CHECK_LAUNCH("bn_stats_fold");
  return GIC_OK;
}

}  // extern "C"
