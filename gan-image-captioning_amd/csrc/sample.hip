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
// The decoders (one step = the recurrence, the vocabulary product into f32 logits, sample_select):
//   LSTM       lstm_step's beam form with parent = own row and token = the sampled token, vocab_step_logits (decoder_step.hip);
//              where the fused kernels decline the shapes, sample_gather + the no-split library GEMMs + LSTM pointwise (beam.hip's
//              generic path with beam width 1)
//   attention  attn_beam.hip's step with K = n and parent = own row: hp GEMM, attn_beam_energy / attn_beam_ctx (an image's fproj / fmap
//              read once for its n rows), lstm_step's beam form, vocab_step_logits
// Once every row has finished, the kernels of each later step read the finished count and return at once (the launch count stays
// fixed; on the generic path the library GEMMs still run on stale rows that nothing reads).
//
// Scratch (one caller-owned workspace, gic_*_sample_ws_bytes; every region 256-byte aligned), rows = B * n:
//   LSTM: xh[l] act [2][rows][Din_l + H], c[l] f32 [2][rows][H] (beam.hip's slots), gpre f32 [rows][4H] (generic path only)
//   attention: xh act [2][rows][E + C + H], c f32 [2][rows][H], fproj act [B][P][A], hp f32 [rows][A], e f32 [rows][P]
//   both: logits f32 [rows][V]; score f32, fin / len / tok / par i32 [rows]; hist_tok i32 [L][rows]; last / done i32 [B]; count i32
#include <climits>

#include "../../include/gicap.h"
#include "beam.h"
#include "kernels.h"

namespace gic {

int lstm_pointwise_fwd(int dt, const float* gpre, const float* c_prev, float* c_new, void* h_next, long ld_next, void* h_up, long ld_up,
                       int rows, int H, hipStream_t stream);      // decoder.hip

namespace {

constexpr int kSampleMax = 8;
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

__global__ __launch_bounds__(kSelThreads) void sample_select_kernel(const SelArgs a) {
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
        if (v < V) f(lr[v], v, -1, e);
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
    for (int e = 0; e < 4; ++e) any |= 4 * q + e < V && okey(l[e]) >= thr;
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
      if (v < V && okey(l[e]) >= thr) {
        const float y = l[e] / tau + gumbel(u[e]);
        if (arg_better(y, v, best, bi)) { best = y; bi = v; }
      }
    }
  };
#pragma unroll
  for (int j = 0; j < kSelQuads; ++j) quad(x[j], tid + j * kSelThreads);
  for (int q = kSelQuads * kSelThreads + tid; q < nq; q += kSelThreads) {
    float l[4];
    for (int e = 0; e < 4; ++e) l[e] = 4 * q + e < V ? lr[4 * q + e] : -INFINITY;
    quad(l, q);
  }
  const int tok = sel_argmax(best, bi, red, ph);
  int nkept = 0;
  if (a.kept) {
    each([&](float l, int, int, int) { nkept += okey(l) >= thr ? 1 : 0; });
    nkept = sel_count(nkept, red, ph);
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

int sample_select(const SelArgs& s, hipStream_t stream) {
  hipLaunchKernelGGL(sample_select_kernel, dim3((unsigned)s.rows), dim3(kSelThreads), 0, stream, s);
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

int sample_finalize(const BeamState& st, int rows, int L, int pad, int64_t* ids, float* scores, int32_t* lengths, hipStream_t stream) {
  hipLaunchKernelGGL(sample_finalize_kernel, dim3((unsigned)cdiv((long)rows * L, 256)), dim3(256), 0, stream, st.score, st.len, st.htok, rows, L,
                     pad, ids, scores, lengths);
  GIC_CHECK_LAUNCH("sample_finalize");
  return GIC_OK;
}

// generic path, t > 0: the GEMM input rows [x | h] of every layer from the previous step's output of the same row, layer 0's x part =
// embed[token]; the cell state likewise (beam.hip's beam_gather with parent = own row)
template <typename TA>
__global__ __launch_bounds__(256) void sample_gather_kernel(BeamLayerPtrs in, BeamLayerPtrs out, int NL, int E, int H, const float* __restrict__ embed,
                                                            const int* __restrict__ tok, const int* stop, int stop_at) {
  if (*stop >= stop_at) return;
  const int r = blockIdx.x, tid = threadIdx.x, id = tok[r];
  for (int l = 0; l < NL; ++l) {
    const int din = l == 0 ? E : H;
    const long ld = din + H;
    TA* dst = (TA*)in.xh[l] + (long)r * ld;
    const TA* src = (const TA*)out.xh[l] + (long)r * ld;
    if (l == 0)
      for (int e = tid; e < E; e += 256) dst[e] = from_f32<TA>(embed[(long)id * E + e]);
    for (int j = tid; j < H; j += 256) {
      dst[din + j] = src[din + j];
      in.c[l][(long)r * H + j] = out.c[l][(long)r * H + j];
    }
  }
}

// the option checks shared by the three entry points (V = the vocabulary)
int check_sample_opts(const gic_sample_opts* o, int V, bool decode, const char* who) {
  GIC_CHECK_ARG(o, "%s: null options", who);
  if (decode) GIC_CHECK_ARG(o->num_samples >= 1 && o->num_samples <= kSampleMax, "%s: num_samples must be 1..%d, got %d", who, kSampleMax, o->num_samples);
  GIC_CHECK_ARG(o->top_k >= 0 && o->top_k <= V, "%s: top_k must be 0..V (%d), got %d", who, V, o->top_k);
  GIC_CHECK_ARG(o->top_p == o->top_p && o->top_p > 0.f && o->top_p <= 1.f, "%s: top_p must be in (0, 1], got %g", who, (double)o->top_p);
  GIC_CHECK_ARG(std::isfinite(o->temperature) && o->temperature > 0.f, "%s: temperature must be finite and > 0, got %g", who, (double)o->temperature);
  if (decode) {
    GIC_CHECK_ARG(o->eos_id >= 0 && o->eos_id < V, "%s: eos_id %d outside [0, %d)", who, o->eos_id, V);
    GIC_CHECK_ARG(o->pad_id >= 0 && o->pad_id < V, "%s: pad_id %d outside [0, %d)", who, o->pad_id, V);
  }
  return GIC_OK;
}

SelArgs sel_step(const float* logits, int rows, int V, const gic_sample_opts* o, const float* noise_u, uint64_t seed, int t,
                 const BeamState& st) {
  SelArgs s{};
  s.logits = logits; s.ld = V; s.rows = rows; s.V = V; s.top_k = o->top_k; s.top_p = o->top_p; s.temperature = o->temperature;
  s.u = noise_u ? noise_u + (long)t * rows * V : nullptr; s.ldu = V;
  s.seed = seed; s.stream = (uint64_t)t;
  s.tok = st.tok; s.fin = st.fin; s.len = st.len; s.score = st.score; s.htok = st.htok + (long)t * rows; s.count = st.count;
  s.eos = o->eos_id; s.t = t;
  return s;
}

// ---------------------------------------------------------------- the LSTM decoder
struct SampleDims {
  int B, L, V, E, H, NL, dt, n, rows;
  bool fused;
  int din(int l) const { return l == 0 ? E : H; }
  long ldx(int l) const { return (long)din(l) + H; }
  size_t asz() const { return (size_t)dtype_size(dt); }
};

struct SampleLayout {
  size_t xh[GIC_MAX_LAYERS], c[GIC_MAX_LAYERS], gpre, logits, score, fin, len, tok, par, htok, last, done, count, total;
};

SampleLayout sample_layout(const SampleDims& d) {
  SampleLayout o{};
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t p = at; at += (bytes + 255) & ~(size_t)255; return p; };
  const size_t R = d.rows;
  for (int l = 0; l < d.NL; ++l) {
    o.xh[l] = take(2 * R * d.ldx(l) * d.asz());
    o.c[l] = take(2 * R * d.H * 4);
  }
  o.gpre = d.fused ? 0 : take(R * 4 * d.H * 4);
  o.logits = take(R * d.V * 4);
  o.score = take(R * 4); o.fin = take(R * 4); o.len = take(R * 4); o.tok = take(R * 4); o.par = take(R * 4);
  o.htok = take((size_t)d.L * R * 4);
  o.last = take((size_t)d.B * 4); o.done = take((size_t)d.B * 4); o.count = take(4);
  o.total = at;
  return o;
}

int sample_dims(const gic_decoder_dims* dims, int n, SampleDims& d) {
  GIC_CHECK_ARG(dims, "decoder_sample: null dims");
  GIC_CHECK_ARG(dims->B > 0 && dims->L > 0 && dims->V > 1 && dims->E > 0 && dims->H > 0, "decoder_sample: bad dims");
  GIC_CHECK_ARG(dims->NL >= 1 && dims->NL <= GIC_MAX_LAYERS, "decoder_sample: gen_num_layers must be 1..%d", GIC_MAX_LAYERS);
  GIC_CHECK_ARG(dims->dtype == DT_F32 || dims->dtype == DT_BF16, "decoder_sample: bad dtype");
  GIC_CHECK_ARG(n >= 1 && n <= kSampleMax, "decoder_sample: num_samples must be 1..%d, got %d", kSampleMax, n);
  GIC_CHECK_ARG(dims->L <= 1024, "decoder_sample: at most 1024 steps");
  GIC_CHECK_ARG((long)dims->B * n <= (1l << 24), "decoder_sample: too many rows");
  d.B = dims->B; d.L = dims->L; d.V = dims->V; d.E = dims->E; d.H = dims->H; d.NL = dims->NL; d.dt = dims->dtype; d.n = n;
  d.rows = d.B * n;
  d.fused = d.rows <= decoder_step_max_rows() && decoder_step_supported(d.dt, d.V, d.E, d.H, d.NL);
  return GIC_OK;
}

template <typename TA>
int decoder_sample_t(const SampleDims& d, const gic_decoder_params* P, const gic_decoder_shadow* S, const gic_sample_opts* o, unsigned char* ws,
                     const float* features, const float* noise_u, uint64_t seed, int64_t* ids, float* scores, int32_t* lengths, hipStream_t stream) {
  const SampleLayout lay = sample_layout(d);
  const int R = d.rows, H = d.H, NL = d.NL;
  BeamLayerPtrs slot[2];
  for (int l = 0; l < NL; ++l)
    for (int s = 0; s < 2; ++s) {
      slot[s].xh[l] = (TA*)(ws + lay.xh[l]) + (long)s * R * d.ldx(l);
      slot[s].c[l] = (float*)(ws + lay.c[l]) + (long)s * R * H;
    }
  float* logits = (float*)(ws + lay.logits);
  const BeamState st{(float*)(ws + lay.score), (int*)(ws + lay.fin), (int*)(ws + lay.len), (int*)(ws + lay.tok), (int*)(ws + lay.par),
                     (int*)(ws + lay.htok), nullptr, (int*)(ws + lay.last), (int*)(ws + lay.done), (int*)(ws + lay.count)};
  GIC_PROPAGATE(beam_init(slot[0], NL, d.E, d.E, H, d.B, d.n, d.dt, features, o->h0, o->c0, st, stream, true));
  for (int t = 0; t < d.L; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    if (d.fused) {
      for (int l = 0; l < NL; ++l) {
        LstmStepArgs a;
        a.xh_t = slot[cur].xh[l]; a.xh_next = slot[nxt].xh[l];
        a.wcat = S->wcat[l]; a.bsum = S->bsum[l];
        a.c_prev = slot[cur].c[l]; a.c_new = slot[nxt].c[l];
        if (l + 1 < NL) { a.h_up = slot[cur].xh[l + 1]; a.ld_up = d.ldx(l + 1); }
        a.B = R; a.H = H; a.din = d.din(l); a.ldx = d.ldx(l);
        a.stop = st.count; a.stop_at = R;
        if (t > 0) {
          a.parent = st.par;                     // = own row
          if (l == 0) { a.gather = 1; a.embed = P->embed; a.V = d.V; a.token = st.tok; }
        }
        GIC_PROPAGATE(lstm_step(a, d.dt, stream));
      }
      VocabStepArgs v;
      v.h = (const TA*)slot[nxt].xh[NL - 1] + d.din(NL - 1); v.ldh = d.ldx(NL - 1);
      v.wout = S->wout; v.bias = P->b_out;
      v.logits = logits; v.ld_logits = d.V;
      v.stop = st.count; v.stop_at = R;
      v.B = R; v.V = d.V; v.H = H;
      GIC_PROPAGATE(vocab_step_logits(v, d.dt, stream));
    } else {
      if (t > 0) {
        hipLaunchKernelGGL((sample_gather_kernel<TA>), dim3((unsigned)R), dim3(256), 0, stream, slot[0], slot[1], NL, d.E, H, P->embed, st.tok,
                           st.count, R);
        GIC_CHECK_LAUNCH("sample_gather");
      }
      float* gpre = (float*)(ws + lay.gpre);
      for (int l = 0; l < NL; ++l) {
        const long ld = d.ldx(l);
        GemmDesc g;
        g.A = slot[0].xh[l]; g.lda = ld; g.B = S->wcat[l]; g.ldb = ld; g.C = gpre; g.ldc = 4 * H;
        g.M = R; g.N = 4 * H; g.K = (int)ld; g.in_dtype = d.dt; g.out_dtype = DT_F32; g.bias = S->bsum[l];
        g.no_split = 1;                          // no split-K atomics: the same bits on every call
        GIC_PROPAGATE(gemm(g, stream));
        GIC_PROPAGATE(lstm_pointwise_fwd(d.dt, gpre, slot[0].c[l], slot[1].c[l], (TA*)slot[1].xh[l] + d.din(l), ld,
                                         l + 1 < NL ? slot[0].xh[l + 1] : nullptr, l + 1 < NL ? d.ldx(l + 1) : 0, R, H, stream));
      }
      GemmDesc g;
      g.A = (const TA*)slot[1].xh[NL - 1] + d.din(NL - 1); g.lda = d.ldx(NL - 1);
      g.B = S->wout; g.ldb = H; g.C = logits; g.ldc = d.V;
      g.M = R; g.N = d.V; g.K = H; g.in_dtype = d.dt; g.out_dtype = DT_F32; g.bias = P->b_out;
      g.no_split = 1;
      GIC_PROPAGATE(gemm(g, stream));
    }
    GIC_PROPAGATE(sample_select(sel_step(logits, R, d.V, o, noise_u, seed, t, st), stream));
  }
  return sample_finalize(st, R, d.L, o->pad_id, ids, scores, lengths, stream);
}

// ---------------------------------------------------------------- the attention decoder
struct AttnSampleDims {
  ACtx c;
  int n, rows;
};

struct AttnSampleLayout {
  size_t xh, c, fproj, hp, e, logits, score, fin, len, tok, par, htok, last, done, count, total;
};

AttnSampleLayout attn_sample_layout(const AttnSampleDims& d) {
  AttnSampleLayout o{};
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t p = at; at += (bytes + 255) & ~(size_t)255; return p; };
  const ACtx& c = d.c;
  const size_t R = d.rows;
  o.xh = take(2 * R * c.ldx() * c.asz());
  o.c = take(2 * R * c.H * 4);
  o.fproj = take((size_t)c.B * c.P * c.A * c.asz());
  o.hp = take(R * c.A * 4);
  o.e = take(R * c.P * 4);
  o.logits = take(R * c.V * 4);
  o.score = take(R * 4); o.fin = take(R * 4); o.len = take(R * 4); o.tok = take(R * 4); o.par = take(R * 4);
  o.htok = take((size_t)c.L * R * 4);
  o.last = take((size_t)c.B * 4); o.done = take((size_t)c.B * 4); o.count = take(4);
  o.total = at;
  return o;
}

int attn_sample_dims(const gic_attn_dims* dims, int n, AttnSampleDims& d) {
  GIC_PROPAGATE(check_attn_dims(dims, d.c));
  GIC_CHECK_ARG(n >= 1 && n <= kSampleMax, "attn_sample: num_samples must be 1..%d, got %d", kSampleMax, n);
  GIC_CHECK_ARG(d.c.L <= 1024, "attn_sample: at most 1024 steps");
  GIC_CHECK_ARG((long)d.c.B * n <= (1l << 24), "attn_sample: too many rows");
  d.n = n;
  d.rows = d.c.B * n;
  return GIC_OK;
}

template <typename TA>
int attn_sample_t(const AttnSampleDims& d, const gic_attn_params* P, const gic_attn_shadow* S, const gic_sample_opts* o, unsigned char* ws,
                  const float* features, const void* fmap, const float* noise_u, uint64_t seed, int64_t* ids, float* scores, int32_t* lengths,
                  hipStream_t stream) {
  const AttnSampleLayout lay = attn_sample_layout(d);
  const ACtx& c = d.c;
  const int R = d.rows, H = c.H, B = c.B;
  const long ldx = c.ldx();
  BeamLayerPtrs slot[2] = {};
  for (int s = 0; s < 2; ++s) {
    slot[s].xh[0] = (TA*)(ws + lay.xh) + (long)s * R * ldx;
    slot[s].c[0] = (float*)(ws + lay.c) + (long)s * R * H;
  }
  const BeamState st{(float*)(ws + lay.score), (int*)(ws + lay.fin), (int*)(ws + lay.len), (int*)(ws + lay.tok), (int*)(ws + lay.par),
                     (int*)(ws + lay.htok), nullptr, (int*)(ws + lay.last), (int*)(ws + lay.done), (int*)(ws + lay.count)};
  void* fproj = ws + lay.fproj;
  float* hp = (float*)(ws + lay.hp);
  float* logits = (float*)(ws + lay.logits);

  GIC_PROPAGATE(beam_init(slot[0], 1, c.din(), c.E, H, B, d.n, c.dt, features, o->h0, o->c0, st, stream, true));
  {  // fp = fmap W_f^T + b_f, once per image
    GemmDesc g;
    g.A = fmap; g.lda = c.C; g.B = S->wf; g.ldb = c.C; g.C = fproj; g.ldc = c.A;
    g.M = B * c.P; g.N = c.A; g.K = c.C; g.in_dtype = c.dt; g.out_dtype = c.dt; g.bias = P->b_f;
    g.no_split = 1;
    GIC_PROPAGATE(gemm(g, stream));
  }
  for (int t = 0; t < c.L; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    TA* xh_t = (TA*)slot[cur].xh[0];
    {  // hp [rows, A] = h_{t-1} W_h^T
      GemmDesc g;
      g.A = xh_t + c.din(); g.lda = ldx; g.B = S->wh; g.ldb = H; g.C = hp; g.ldc = c.A;
      g.M = R; g.N = c.A; g.K = H; g.in_dtype = c.dt; g.out_dtype = DT_F32;
      g.no_split = 1;
      GIC_PROPAGATE(gemm(g, stream));
    }
    AttnBeamArgs f;
    f.fproj = fproj; f.fmap = fmap; f.w_a = P->w_a; f.hp = hp; f.par = st.par; f.e = (float*)(ws + lay.e);
    f.z = xh_t + c.E; f.ldx = ldx; f.alpha = nullptr;
    f.stop = st.count; f.stop_at = R;
    f.P = c.P; f.A = c.A; f.C = c.C;
    GIC_PROPAGATE(attn_beam_step(f, d.n, B, c.dt, stream));
    LstmStepArgs a;
    a.xh_t = xh_t; a.xh_next = slot[nxt].xh[0]; a.wcat = S->wcat; a.bsum = S->bsum;
    a.c_prev = slot[cur].c[0]; a.c_new = slot[nxt].c[0];
    a.B = R; a.H = H; a.din = c.din(); a.ldx = ldx; a.gw = c.E;
    a.stop = st.count; a.stop_at = R;
    if (t > 0) { a.parent = st.par; a.gather = 1; a.embed = P->embed; a.V = c.V; a.token = st.tok; }
    GIC_PROPAGATE(lstm_step(a, c.dt, stream));
    VocabStepArgs v;
    v.h = (const TA*)slot[nxt].xh[0] + c.din(); v.ldh = ldx;
    v.wout = S->wout; v.bias = P->b_out;
    v.logits = logits; v.ld_logits = c.V;
    v.stop = st.count; v.stop_at = R;
    v.B = R; v.V = c.V; v.H = H;
    GIC_PROPAGATE(vocab_step_logits(v, c.dt, stream));
    GIC_PROPAGATE(sample_select(sel_step(logits, R, c.V, o, noise_u, seed, t, st), stream));
  }
  return sample_finalize(st, R, c.L, o->pad_id, ids, scores, lengths, stream);
}

}  // namespace
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

int gic_decoder_sample_ws_bytes(const gic_decoder_dims* dims, int32_t num_samples, uint64_t* out) {
  SampleDims d;
  GIC_PROPAGATE(sample_dims(dims, num_samples, d));
  GIC_CHECK_ARG(out, "decoder_sample_ws_bytes: null out");
  *out = (uint64_t)sample_layout(d).total;
  return GIC_OK;
}

int gic_decoder_sample_captions(const gic_decoder_dims* dims, const gic_decoder_params* P, const gic_decoder_shadow* S, const gic_sample_opts* o,
                                void* ws, const float* features, const float* noise_u, uint64_t seed, int64_t* ids, float* scores,
                                int32_t* lengths, void* stream) {
  GIC_CHECK_ARG(o, "decoder_sample_captions: null options");
  SampleDims d;
  GIC_PROPAGATE(sample_dims(dims, o->num_samples, d));
  GIC_PROPAGATE(check_sample_opts(o, d.V, true, "decoder_sample_captions"));
  GIC_CHECK_ARG(P && S && ws && features && ids && scores && lengths, "decoder_sample_captions: null argument");
  GIC_CHECK_ARG(P->embed && P->b_out && S->wout, "decoder_sample_captions: null embedding / output layer");
  for (int l = 0; l < d.NL; ++l) GIC_CHECK_ARG(S->wcat[l] && S->bsum[l], "decoder_sample_captions: null layer %d weights", l);
  GIC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "decoder_sample_captions: the workspace must be 256-byte aligned");
  if (d.dt == DT_F32)
    return decoder_sample_t<float>(d, P, S, o, (unsigned char*)ws, features, noise_u, seed, ids, scores, lengths, (hipStream_t)stream);
  return decoder_sample_t<bf16_t>(d, P, S, o, (unsigned char*)ws, features, noise_u, seed, ids, scores, lengths, (hipStream_t)stream);
}

int gic_attn_sample_ws_bytes(const gic_attn_dims* dims, int32_t num_samples, uint64_t* out) {
  AttnSampleDims d;
  GIC_PROPAGATE(attn_sample_dims(dims, num_samples, d));
  GIC_CHECK_ARG(out, "attn_sample_ws_bytes: null out");
  *out = (uint64_t)attn_sample_layout(d).total;
  return GIC_OK;
}

int gic_attn_sample_captions(const gic_attn_dims* dims, const gic_attn_params* P, const gic_attn_shadow* S, const gic_sample_opts* o, void* ws,
                             const float* features, const void* fmap, const float* noise_u, uint64_t seed, int64_t* ids, float* scores,
                             int32_t* lengths, void* stream) {
  GIC_CHECK_ARG(o, "attn_sample_captions: null options");
  AttnSampleDims d;
  GIC_PROPAGATE(attn_sample_dims(dims, o->num_samples, d));
  GIC_PROPAGATE(check_sample_opts(o, d.c.V, true, "attn_sample_captions"));
  GIC_CHECK_ARG(P && S && ws && features && fmap && ids && scores && lengths, "attn_sample_captions: null argument");
  GIC_CHECK_ARG(P->embed && P->b_out && P->b_f && P->w_a && S->wcat && S->bsum && S->wout && S->wf && S->wh, "attn_sample_captions: null weights");
  GIC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "attn_sample_captions: the workspace must be 256-byte aligned");
  if (d.c.dt == DT_F32)
    return attn_sample_t<float>(d, P, S, o, (unsigned char*)ws, features, fmap, noise_u, seed, ids, scores, lengths, (hipStream_t)stream);
  return attn_sample_t<bf16_t>(d, P, S, o, (unsigned char*)ws, features, fmap, noise_u, seed, ids, scores, lengths, (hipStream_t)stream);
}

}  // extern "C"
