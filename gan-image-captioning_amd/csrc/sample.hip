// Caption sampling (gicap.h gic_sample_logits, gic_decoder_sample_captions, gic_attn_sample_captions): temperature / top-k / top-p
// draws of n captions per image.  Rows = B * n (row r = image r / n, sample r % n), every row live from step 0.
//
// sample_select: one workgroup (512 threads) per row.  The row's f32 logits are read once into registers (8 quads per thread: rows
// up to 16384 entries; entries beyond stream from L2 on every pass).  Then, all from registers:
//   max m, logsumexp at tau = 1 (the score), and with top-p e_v = exp((l_v - m) / tau) over the top-k set
//   top-k boundary   bisection over the order-preserving 32-bit key of l: the largest key T with #{key >= T} >= k (integer counts;
//                    a pass whose count is exactly k ends the search, the set is then final)
//   top-p boundary   bisection over the same key: the largest T with sum_{key >= T} e >= top_p * sum e (the top-k set's masses)
//   draw             argmax over kept v of l_v / tau + gumbel(u_v), ties to the lower id; u explicit or Philox(seed, stream, (r, quad))
// Every block reduction is a wave butterfly then the 8 wave values added in wave order: no LDS or global f32 atomics, so the
// boundaries do not depend on the order in which waves arrive, and two calls give the same bits.
//
// The samplers (gic_decoder_sample_captions, gic_attn_sample_captions) are decode.hip's step loop with this head: the vocabulary product
// into f32 logits (vocab_step_logits, or the library GEMM on the LSTM generic path), then sample_step; sample_finalize after the last
// step.  Every row is live from step 0 and is its own parent.
#include <climits>

#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {
namespace {

constexpr int kSelThreads = 512;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelQuads = 8;                     // quads of logits per thread held in registers: 512 * 8 * 4 = 16384 entries

struct SelArgs {
  const float* logits; long ld;                  // f32 [rows][ld]
  int rows, V, top_k;
  float top_p, temperature;
  const float* u; long ldu;                      // explicit uniforms, row r at u + r * ldu, or null -> Philox(seed, stream, r * nq + quad)
  uint64_t seed, stream;
  int64_t* ids; float* logp; int32_t* kept;      // gic_sample_logits' outputs (null in the decoders)
  int* tok; int* fin; int* len; float* score;    // decode state (null for gic_sample_logits)
  int* htok; int* count;                         // this step's history slot [rows]; the finished count (also the stop flag)
  int eos, t;
};

// decode constraints, the BAN kernel's own argument (SelArgs, and with it sample_select_kernel's argument layout, stay as they were)
struct SelBan {
  BanLists bans;                                 // the row's banned ids leave the kept set
  BanOut bout; BanRule rule;                     // and the kernel's tail builds the row's list of step t + 1 (bout.nban / ban; hist unused)
  const int* hbase = nullptr;                    // the history [L][rows] whose slot t is SelArgs::htok
};

// unsigned order of the keys = float order of the values; -0 and +0 share a key, as they are equal values (NaN never occurs in
// logits that came from finite weights)
__device__ __forceinline__ unsigned okey(float x) {
  const unsigned b = x == 0.f ? 0u : __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float gumbel(float u) { return -logf(-logf(u + 1e-10f) + 1e-10f); }    // generator.py:84-96

// block reductions: a wave butterfly (every lane ends with the same bits), then the wave values in wave order; two LDS buffers
// alternate, so a reduction needs one barrier (the next one that reuses a buffer is two barriers later)
struct SelRed {
  float f[2][kSelWaves];
  int i[2][kSelWaves];
};

__device__ __forceinline__ float sel_sum(float v, SelRed& s, int& ph) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s.f[ph][threadIdx.x >> 6] = v;
  __syncthreads();
  float t = s.f[ph][0];
#pragma unroll
  for (int w = 1; w < kSelWaves; ++w) t += s.f[ph][w];
  ph ^= 1;
  return t;
}

__device__ __forceinline__ float sel_max(float v, SelRed& s, int& ph) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) s.f[ph][threadIdx.x >> 6] = v;
  __syncthreads();
  float t = s.f[ph][0];
#pragma unroll
  for (int w = 1; w < kSelWaves; ++w) t = fmaxf(t, s.f[ph][w]);
  ph ^= 1;
  return t;
}

__device__ __forceinline__ int sel_count(int v, SelRed& s, int& ph) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s.i[ph][threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < kSelWaves; ++w) t += s.i[ph][w];
  ph ^= 1;
  return t;
}

// (value, index) argmax, ties to the lower index; index INT_MAX = no candidate
__device__ __forceinline__ bool arg_better(float v, int i, float w, int j) { return j == INT_MAX || (i != INT_MAX && (v > w || (v == w && i < j))); }

__device__ __forceinline__ int sel_argmax(float v, int i, SelRed& s, int& ph) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (arg_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
  if ((threadIdx.x & 63) == 0) { s.f[ph][threadIdx.x >> 6] = v; s.i[ph][threadIdx.x >> 6] = i; }
  __syncthreads();
  float bv = s.f[ph][0];
  int bi = s.i[ph][0];
#pragma unroll
  for (int w = 1; w < kSelWaves; ++w)
    if (arg_better(s.f[ph][w], s.i[ph][w], bv, bi)) { bv = s.f[ph][w]; bi = s.i[ph][w]; }
  ph ^= 1;
  return bi;
}

// BAN: after the score's logsumexp (over the raw values) the entries of the row's ban list become -inf, before the top-k / top-p
// bisections and the draw; the max under top-p's exponent is then the admissible entries' own.  The workgroup owns its row and its
// history, so once the token is drawn its first wave builds the row's list of the next step (unless the row has just finished)
struct NoBan {};

template <bool BAN, typename Ban>
__global__ __launch_bounds__(kSelThreads) void sample_select_kernel(const SelArgs a, const Ban c) {
  __shared__ SelRed red;
  int ph = 0;
  const int r = blockIdx.x, tid = threadIdx.x, V = a.V;
  if (a.count) {
    if (*a.count >= a.rows) return;              // every row has finished: the step is the identity
    if (a.fin[r]) return;                        // this row has: its score, length and history stay as they are
  }
  const float* lr = a.logits + (long)r * a.ld;
  const int nq = (V + 3) >> 2;                   // quads of the row; quad q = entries 4q .. 4q + 3
  float x[kSelQuads][4];
#pragma unroll
  for (int j = 0; j < kSelQuads; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = 4 * (tid + j * kSelThreads) + e;
      x[j][e] = v < V ? lr[v] : -INFINITY;
    }
  int nb = 0;
  const int* bl = nullptr;
  if constexpr (BAN) {
    nb = c.bans.nban[r];
    bl = c.bans.ban + (long)r * c.bans.cap;      // (read from L2 as it is: staging it in LDS measured slower)
  }
  bool masked = false;                           // BAN: the banned entries read as -inf from here on
  auto streamed = [&](int v) {                   // an entry beyond the registers
    float l = lr[v];
    if constexpr (BAN) {
      if (masked)
        for (int i = 0; i < nb; ++i) l = bl[i] == v ? -INFINITY : l;
    }
    return l;
  };
  // f(l, v, j, e) for every entry of the row this thread holds; j < 0 for the streamed entries beyond the registers
  auto each = [&](auto&& f) {
#pragma unroll
    for (int j = 0; j < kSelQuads; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = 4 * (tid + j * kSelThreads) + e;
        if (v < V) f(x[j][e], v, j, e);
      }
    for (int q = kSelQuads * kSelThreads + tid; q < nq; q += kSelThreads)
      for (int e = 0; e < 4; ++e) {
        const int v = 4 * q + e;
        if (v < V) f(streamed(v), v, -1, e);
      }
  };

  // ---- max and logsumexp at tau = 1
  float m = -INFINITY;
  each([&](float l, int, int, int) { m = fmaxf(m, l); });
  m = sel_max(m, red, ph);
  float s1 = 0.f;
  each([&](float l, int, int, int) { s1 += expf(l - m); });
  const float lse = m + logf(sel_sum(s1, red, ph));
  const float tau = a.temperature;
  if constexpr (BAN) {
    for (int i = 0; i < nb; ++i) {
      const int b = bl[i], q = b >> 2;
      if (q % kSelThreads != tid) continue;
#pragma unroll
      for (int j = 0; j < kSelQuads; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (q / kSelThreads == j && (b & 3) == e) x[j][e] = -INFINITY;
    }
    masked = true;
    m = -INFINITY;
    each([&](float l, int, int, int) { m = fmaxf(m, l); });
    m = sel_max(m, red, ph);
  }

  // ---- top-k: the largest key T with #{key >= T} >= k
  unsigned thr = 0u;
  if (a.top_k > 0 && a.top_k < V) {
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned c = thr | (1u << bit);
      int n = 0;
      each([&](float l, int, int, int) { n += okey(l) >= c ? 1 : 0; });
      n = sel_count(n, red, ph);
      if (n >= a.top_k) {
        thr = c;
        if (n == a.top_k) break;                 // {key >= c} is exactly the top k: raising T further keeps the same set
      }
    }
  }
  // ---- top-p over the top-k set: the largest key T with sum_{key >= T} e >= top_p * sum e
  if (a.top_p < 1.f) {
    float ex[kSelQuads][4];
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < kSelQuads; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) ex[j][e] = okey(x[j][e]) >= thr ? expf((x[j][e] - m) / tau) : 0.f;
    each([&](float l, int, int j, int e) { z += j >= 0 ? ex[j][e] : (okey(l) >= thr ? expf((l - m) / tau) : 0.f); });
    const float goal = a.top_p * sel_sum(z, red, ph);
    unsigned tp = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned c = tp | (1u << bit);
      float mass = 0.f;
      each([&](float l, int, int j, int e) {
        const unsigned k = okey(l);
        if (k >= c) mass += j >= 0 ? ex[j][e] : (k >= thr ? expf((l - m) / tau) : 0.f);
      });
      if (sel_sum(mass, red, ph) >= goal) tp = c;
    }
    thr = max(thr, tp);
  }

  // ---- draw: argmax over the kept entries of l / tau + gumbel(u)
  float best = -INFINITY;
  int bi = INT_MAX;
  auto quad = [&](const float (&l)[4], int q) {
    bool any = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) any |= 4 * q + e < V && okey(l[e]) >= thr && (!BAN || l[e] != -INFINITY);
    if (!any) return;
    float u[4];
    if (a.u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) u[e] = 4 * q + e < V ? a.u[(long)r * a.ldu + 4 * q + e] : 0.f;
    } else {
      uint32_t r0, r1, r2, r3;
      Philox::gen4(a.seed, a.stream, (uint64_t)r * (uint64_t)nq + (uint64_t)q, r0, r1, r2, r3);
      u[0] = Philox::u01(r0); u[1] = Philox::u01(r1); u[2] = Philox::u01(r2); u[3] = Philox::u01(r3);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = 4 * q + e;
      if (v < V && okey(l[e]) >= thr && (!BAN || l[e] != -INFINITY)) {
        const float y = l[e] / tau + gumbel(u[e]);
        if (arg_better(y, v, best, bi)) { best = y; bi = v; }
      }
    }
  };
#pragma unroll
  for (int j = 0; j < kSelQuads; ++j) quad(x[j], tid + j * kSelThreads);
  for (int q = kSelQuads * kSelThreads + tid; q < nq; q += kSelThreads) {
    float l[4];
    for (int e = 0; e < 4; ++e) l[e] = 4 * q + e < V ? streamed(4 * q + e) : -INFINITY;
    quad(l, q);
  }
  const int tok = sel_argmax(best, bi, red, ph);
  int nkept = 0;
  if (a.kept) {
    each([&](float l, int, int, int) { nkept += okey(l) >= thr ? 1 : 0; });
    nkept = sel_count(nkept, red, ph);
  }
  if constexpr (BAN) {
    __shared__ int hs[1024];                     // (L <= 1024: decode_dims)
    const int tn = a.t + 1;                      // tokens emitted so far
    const bool next = tn < c.bout.L && tok != a.eos;          // (block-uniform: every thread holds the drawn token)
    if (next && tid < 64)
      for (int i = tid; i < tn; i += 64) hs[i] = i < a.t ? c.hbase[(long)i * a.rows + r] : tok;
    __syncthreads();
    if (next && tid < 64) ban_list_wave(hs, tn, tid, c.rule, c.bout.ban + (long)r * c.bout.cap, c.bout.nban + r);
  }
  if (tid != 0) return;
  const float lp = lr[tok] - lse;
  if (a.ids) a.ids[r] = tok;
  if (a.logp) a.logp[r] = lp;
  if (a.kept) a.kept[r] = nkept;
  if (a.tok) {
    a.tok[r] = tok;
    a.htok[r] = tok;
    a.score[r] += lp;
    a.len[r] = a.t + 1;
    if (tok == a.eos) {
      a.fin[r] = 1;
      atomicAdd(a.count, 1);                     // (integer count: the later launches of the decode return at once)
    }
  }
}

int sample_select(const SelArgs& s, hipStream_t stream, const SelBan& c = SelBan()) {
  if (c.bans.nban) hipLaunchKernelGGL((sample_select_kernel<true, SelBan>), dim3((unsigned)s.rows), dim3(kSelThreads), 0, stream, s, c);
  else hipLaunchKernelGGL((sample_select_kernel<false, NoBan>), dim3((unsigned)s.rows), dim3(kSelThreads), 0, stream, s, NoBan());
  GIC_CHECK_LAUNCH("sample_select");
  return GIC_OK;
}

// ids [rows][L] = the history up to each row's length, pad_id behind; scores / lengths [rows]
__global__ __launch_bounds__(256) void sample_finalize_kernel(const float* __restrict__ score, const int* __restrict__ len,
                                                              const int* __restrict__ htok, int rows, int L, int pad, int64_t* __restrict__ ids,
                                                              float* __restrict__ scores, int32_t* __restrict__ lengths) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)rows * L) return;
  const int r = (int)(i / L), t = (int)(i % L);
  const int n = len[r];
  ids[i] = t < n ? htok[(long)t * rows + r] : pad;
  if (t == 0) { scores[r] = score[r]; lengths[r] = n; }
}

}  // namespace

int sample_finalize(const BeamState& st, int rows, int L, int pad, int64_t* ids, float* scores, int32_t* lengths, hipStream_t stream) {
  hipLaunchKernelGGL(sample_finalize_kernel, dim3((unsigned)cdiv((long)rows * L, 256)), dim3(256), 0, stream, st.score, st.len, st.htok, rows, L,
                     pad, ids, scores, lengths);
  GIC_CHECK_LAUNCH("sample_finalize");
  return GIC_OK;
}

int check_sample_opts(const gic_sample_opts* o, int V, bool decode, const char* who) {
  GIC_CHECK_ARG(o, "%s: null options", who);
  GIC_CHECK_ARG(o->top_k >= 0 && o->top_k <= V, "%s: top_k must be 0..V (%d), got %d", who, V, o->top_k);
  GIC_CHECK_ARG(o->top_p == o->top_p && o->top_p > 0.f && o->top_p <= 1.f, "%s: top_p must be in (0, 1], got %g", who, (double)o->top_p);
  GIC_CHECK_ARG(std::isfinite(o->temperature) && o->temperature > 0.f, "%s: temperature must be finite and > 0, got %g", who, (double)o->temperature);
  if (decode) {
    GIC_CHECK_ARG(o->eos_id >= 0 && o->eos_id < V, "%s: eos_id %d outside [0, %d)", who, o->eos_id, V);
    GIC_CHECK_ARG(o->pad_id >= 0 && o->pad_id < V, "%s: pad_id %d outside [0, %d)", who, o->pad_id, V);
  }
  return GIC_OK;
}

int sample_step(const float* logits, int rows, int V, const gic_sample_opts* o, const float* noise_u, uint64_t seed, int t, const BeamState& st,
                hipStream_t stream, const BanLists& bans, const BanOut& out, const BanRule& rule) {
  SelArgs s{};
  s.logits = logits; s.ld = V; s.rows = rows; s.V = V; s.top_k = o->top_k; s.top_p = o->top_p; s.temperature = o->temperature;
  s.u = noise_u ? noise_u + (long)t * rows * V : nullptr; s.ldu = V;
  s.seed = seed; s.stream = (uint64_t)t;
  s.tok = st.tok; s.fin = st.fin; s.len = st.len; s.score = st.score; s.htok = st.htok + (long)t * rows; s.count = st.count;
  s.eos = o->eos_id; s.t = t;
  SelBan c;
  c.bans = bans; c.bout = out; c.rule = rule; c.hbase = st.htok;
  return sample_select(s, stream, c);
}

}  // namespace gic

using namespace gic;

extern "C" {

int gic_sample_logits(const float* logits, int64_t ld, int32_t rows, int32_t V, const gic_sample_opts* o, const float* noise_u, uint64_t seed,
                      uint64_t stream_id, int64_t* ids, float* logp, int32_t* kept, void* stream) {
  GIC_CHECK_ARG(rows >= 1 && rows <= (1 << 24) && V >= 2 && ld >= V, "sample_logits: bad shape (rows %d, V %d, ld %lld)", rows, V, (long long)ld);
  GIC_PROPAGATE(check_sample_opts(o, V, false, "sample_logits"));
  GIC_CHECK_ARG(logits && ids, "sample_logits: null argument");
  SelArgs s{};
  s.logits = logits; s.ld = ld; s.rows = rows; s.V = V; s.top_k = o->top_k; s.top_p = o->top_p; s.temperature = o->temperature;
  s.u = noise_u; s.ldu = V; s.seed = seed; s.stream = stream_id;
  s.ids = ids; s.logp = logp; s.kept = kept;
  return sample_select(s, (hipStream_t)stream);
}

}  // extern "C"
