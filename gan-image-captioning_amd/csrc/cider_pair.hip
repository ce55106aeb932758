// Pairwise CIDEr-D among the K captions of an image (gicap.h gic_cider_pairwise): the K x K matrix M[i][j] = CIDEr-D of caption i against
// caption j as its single reference, the row consensus (minimum-Bayes-risk selection) and the Self-CIDEr diversity (Wang & Chan 2019) of
// the set, with the tokens, vectors, idf table and length of cider.hip.  DESIGN.md section 23.
//
// One workgroup (8 waves) per image; a caption position is a lane (lengths <= 64 = the wave width).
//   1. captions   each wave strips one caption's specials by a ballot compaction into its own LDS row and stores the 4-token window of
//                 every position (caption_tokens.h): win[k][p].
//   2. vectors    one wave per caption, n = 1..4 side by side: lane p owns the n-grams at p; one is the first occurrence when no earlier
//                 position holds the same key, its count is the number of positions that do; first occurrences look their idf up by
//                 binary search in the global table, the four searches of a lane in lock-step (a search is a chain of dependent
//                 global loads, the one long latency of this kernel: a wave per (caption, n) would walk them one after the other).
//                 wgt[k][p][n-1] = count * idf (0 at every other position, and past the caption's n-grams),
//                 norm[k][n-1] = sqrt(wave sum of wgt^2).  Every caption's vectors are built here, once.
//   3. pairs      the unordered pairs {i, j}, i < j, go round the waves.  Lane p holds caption i's window and four weights and walks
//                 caption j's positions q (one 8-byte and one 16-byte LDS broadcast per q): v_j of lane p's n-gram is the sum of j's
//                 weights over the positions whose first n tokens equal p's -- one non-zero term, the first occurrence's, so the sum
//                 is exact.  With a = min(v_i, v_j), wave sums of a v_j give M[i][j] and of a v_i give M[j][i] from the one pass.
//                 The diagonal comes from the norms: 2.5 per non-zero vector.
//   4. outputs    from the matrix in LDS: the row consensus (j ascending), S = (M + M^T) / 20, and lambda_max(S) by
//                 GIC_CIDER_PAIR_SQUARINGS trace-normalised squarings of S followed by the Rayleigh quotient of S at the power's row
//                 sums (2^squarings power steps from the all-ones vector; always that many, whatever the spectrum).
// LDS, static, sized for K = 32: 16 KB of windows, 32 KB of weights, 4.1 KB of matrix (rows padded to 33), 2.1 KB of token rows, norms
// and lengths: 56192 bytes (54.9 KB) of the 64 KB a kernel gets without asking.  The squaring buffers (3 x 4.1 KB and two vectors) reuse the weights,
// which are dead by then.  Banking: a wave reads its own caption's row p-contiguous (8 B x 64 lanes = both bank rows once, 16 B x 64 in four
// conflict-free groups) and the other caption's position q at one address for all lanes (a broadcast), so the [K][64] rows need no padding.
// Every sum is a wave butterfly or a loop in a fixed order, no atomics: two calls give the same bits, in deterministic mode too.
#include <cmath>

#include "../../include/gicap.h"
#include "caption_tokens.h"
#include "common.h"

namespace gic {
namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / WAVE;
constexpr int kMaxLen = GIC_CIDER_MAX_LEN;          // = WAVE: lane p is position p
constexpr int kMaxK = GIC_CIDER_PAIR_MAX_K;
constexpr int kLd = kMaxK + 1;                      // row stride of the K x K matrices: a column walk touches every bank once
constexpr int kSquarings = GIC_CIDER_PAIR_SQUARINGS;
static_assert(kMaxLen == WAVE, "a caption position is a lane");
static_assert((3 * kMaxK * kLd + 2 * kMaxK) * sizeof(float) <= sizeof(f32x4) * kMaxK * kMaxLen, "the squaring buffers live in the weights");

struct PairArgs {
  const int64_t* ids; long ld; const int32_t* len; int K, L;
  const uint64_t* keys; const float* idf; long n_keys; float log_n;
  float* matrix; float* consensus; float* self_cider;
};

// lookup_idf of a lane's four keys in lock-step (where own[c]; 0 elsewhere): each search is a chain of ~log2(n_keys) dependent global
// loads, and four independent chains in flight hide each other's latency.  Every chain makes lookup_idf's comparisons: bit_length(n_keys)
// rounds end each of them, and a chain that has ended loads keys[0] and ignores it, so the four loads of a round need no branch.
__device__ __forceinline__ void lookup_idf4(const uint64_t (&key)[4], const bool (&own)[4], const uint64_t* keys, const float* idf,
                                            long n_keys, float log_n, float (&out)[4]) {
  long lo[4], hi[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { lo[c] = 0; hi[c] = own[c] ? n_keys : 0; }
  for (long span = n_keys; span > 0; span >>= 1) {
    uint64_t at[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) at[c] = keys[lo[c] < hi[c] ? (lo[c] + hi[c]) >> 1 : 0];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (lo[c] < hi[c]) {
        const long mid = (lo[c] + hi[c]) >> 1;
        if (at[c] < key[c]) lo[c] = mid + 1; else hi[c] = mid;
      }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const bool in = own[c] && lo[c] < n_keys;       // (n_keys = 0: nothing is read)
    const long at = in ? lo[c] : 0;
    out[c] = !own[c] ? 0.f : (in && keys[at] == key[c]) ? idf[at] : log_n;
  }
}

__global__ __launch_bounds__(kThreads) void cider_pair_kernel(const PairArgs a) {
  __shared__ uint64_t win[kMaxK][kMaxLen];
  __shared__ f32x4 wgt[kMaxK][kMaxLen];
  __shared__ float M[kMaxK][kLd];
  __shared__ float norm[kMaxK][4];
  __shared__ int clen[kMaxK];
  __shared__ int tok[kWaves][kMaxLen + 4];
  const int b = blockIdx.x, K = a.K, tid = threadIdx.x, wave = tid / WAVE, lane = tid & (WAVE - 1);

  // 1. captions: stripped tokens, then the 4-token window of every position
  for (int k = wave; k < K; k += kWaves) {
    const long row = (long)b * K + k;
    const int len = min(max(a.len[row], 0), a.L);
    const int cnt = strip_row(a.ids + row * a.ld, len, tok[wave]);
    win[k][lane] = window(tok[wave], lane);
    if (lane == 0) clen[k] = cnt;
    wave_lds_sync();                                // the windows are read before the next caption's tokens land
  }
  __syncthreads();

  // 2. per caption, its four orders side by side: the idf-weighted counts at the first occurrences, and their norms
  for (int k = wave; k < K; k += kWaves) {
    const uint64_t wk = win[k][lane];
    const int len = clen[k];
    int cnt[4] = {0, 0, 0, 0};
    bool own[4] = {true, true, true, true};
    for (int q = 0; q < len; ++q) {                 // a window past the n-grams' end holds a zero token: it equals no n-gram of the caption
      const uint64_t x = wk ^ win[k][q];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const bool eq = (x >> (15 * (3 - n))) == 0;
        cnt[n] += eq;
        own[n] = own[n] && !(eq && q < lane);
      }
    }
    uint64_t key[4];
    float idf[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      own[n] = own[n] && lane < len - n;            // the caption has len - n (n + 1)-grams
      key[n] = ngram_key(wk, n + 1);
    }
    lookup_idf4(key, own, a.keys, a.idf, a.n_keys, a.log_n, idf);
    f32x4 v;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      v[n] = own[n] ? (float)cnt[n] * idf[n] : 0.f;
      const float v2 = wave_sum(v[n] * v[n]);
      if (lane == 0) norm[k][n] = sqrtf(v2);
    }
    wgt[k][lane] = v;
  }
  __syncthreads();

  // 3. the diagonal from the norms, then one matching pass per unordered pair
  if (tid < K) {
    int nz = 0;
    for (int n = 0; n < 4; ++n) nz += norm[tid][n] != 0.f;
    M[tid][tid] = 2.5f * (float)nz;
  }
  for (int p = wave; p < K * (K - 1) / 2; p += kWaves) {
    int i = 0, rem = p;
    while (rem >= K - 1 - i) { rem -= K - 1 - i; ++i; }                        // pair p in the order (0,1) (0,2) .. (1,2) ..
    const int j = i + 1 + rem;
    const uint64_t wi = win[i][lane];
    const f32x4 vi = wgt[i][lane];
    f32x4 vj = {0.f, 0.f, 0.f, 0.f};
    const int mj = clen[j];
    for (int q = 0; q < mj; ++q) {
      const uint64_t x = wi ^ win[j][q];                                        // the first n tokens agree: the top 15 n bits are zero
      const f32x4 wj = wgt[j][q];
      if ((x >> 45) == 0) vj[0] += wj[0];
      if ((x >> 30) == 0) vj[1] += wj[1];
      if ((x >> 15) == 0) vj[2] += wj[2];
      if (x == 0) vj[3] += wj[3];
    }
    const float delta = (float)(max(clen[i] - 1, 0) - max(mj - 1, 0));          // "length" = the number of bigrams
    const float pen = expf(-(delta * delta) / kCiderTwoSigma2);
    float acc_ij = 0.f, acc_ji = 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const float m = fminf(vi[n], vj[n]);
      float dij = wave_sum(m * vj[n]), dji = wave_sum(m * vi[n]);
      const float ni = norm[i][n], nj = norm[j][n];
      if (ni != 0.f && nj != 0.f) { dij /= ni * nj; dji /= nj * ni; }
      acc_ij += dij * pen;
      acc_ji += dji * pen;
    }
    if (lane == 0) {
      M[i][j] = acc_ij / 4.f * 10.f;
      M[j][i] = acc_ji / 4.f * 10.f;
    }
  }
  __syncthreads();

  // 4. outputs
  if (a.matrix)
    for (int e = tid; e < K * K; e += kThreads) a.matrix[(long)b * K * K + e] = M[e / K][e % K];
  if (a.consensus && tid < K) {
    float s = 0.f;
    for (int j = 0; j < K; ++j)
      if (j != tid) s += M[tid][j];
    a.consensus[(long)b * K + tid] = K > 1 ? s / (float)(K - 1) : 0.f;
  }
  if (!a.self_cider) return;

  float* S = reinterpret_cast<float*>(&wgt[0][0]);                              // the weights are dead: S, two power buffers, v, S v
  float* X0 = S + kMaxK * kLd;
  float* X1 = X0 + kMaxK * kLd;
  float* v = X1 + kMaxK * kLd;
  float* w = v + kMaxK;
  for (int e = tid; e < K * K; e += kThreads) {
    const int r = e / K, c = e % K;
    const float s = (M[r][c] + M[c][r]) / 20.f;
    S[r * kLd + c] = s;
    X0[r * kLd + c] = s;
  }
  __syncthreads();
  float tr = 0.f;
  for (int r = 0; r < K; ++r) tr += S[r * kLd + r];                             // every thread forms the same sum
  if (K == 1 || !(tr > 0.f)) {
    if (tid == 0) a.self_cider[b] = 0.f;
    return;
  }
  // X <- (X / trace X)^2, kSquarings times: X / trace X = S^(2^t) / trace(S^(2^t)), its entries within [-1, 1] and its trace 1, so the
  // next trace lies in [1/K, 1]: nothing overflows or vanishes
  float scale = 1.f / tr;
  for (int t = 0; t < kSquarings; ++t) {
    const float* src = (t & 1) ? X1 : X0;
    float* dst = (t & 1) ? X0 : X1;
    const float s2 = scale * scale;
    for (int e = tid; e < K * K; e += kThreads) {
      const int r = e / K, c = e % K;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc += src[r * kLd + k] * src[k * kLd + c];
      dst[r * kLd + c] = acc * s2;
    }
    __syncthreads();
    float t1 = 0.f;
    for (int r = 0; r < K; ++r) t1 += dst[r * kLd + r];
    scale = 1.f / t1;
  }
  const float* P = (kSquarings & 1) ? X1 : X0;
  if (tid < K) {
    float s = 0.f;
    for (int c = 0; c < K; ++c) s += P[tid * kLd + c];
    v[tid] = s;
  }
  __syncthreads();
  if (tid < K) {
    float s = 0.f;
    for (int c = 0; c < K; ++c) s += S[tid * kLd + c] * v[c];
    w[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float num = 0.f, den = 0.f;
    for (int i = 0; i < K; ++i) { num += v[i] * w[i]; den += v[i] * v[i]; }
    const float sc = -logf(num / den / tr) / logf((float)K);
    a.self_cider[b] = fminf(fmaxf(sc, 0.f), 1.f);                               // S need not be positive semi-definite: the clamp
  }
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" {

int gic_cider_pairwise(const int64_t* ids, int64_t ld_ids, const int32_t* lengths, int32_t B, int32_t K, int32_t L, const uint64_t* keys,
                       const float* idf, int64_t n_keys, float log_n, int32_t V, float* matrix, float* consensus, float* self_cider,
                       void* stream) {
  GIC_CHECK_ARG(K >= 1 && K <= GIC_CIDER_PAIR_MAX_K, "cider_pairwise: K=%d outside 1..%d captions per image", K, GIC_CIDER_PAIR_MAX_K);
  GIC_CHECK_ARG(L >= 1 && L <= GIC_CIDER_MAX_LEN, "cider_pairwise: L=%d outside 1..%d ids per caption", L, GIC_CIDER_MAX_LEN);
  GIC_CHECK_ARG(V >= 1 && V <= GIC_CIDER_MAX_VOCAB, "cider_pairwise: V=%d outside 1..%d (15-bit n-gram keys)", V, GIC_CIDER_MAX_VOCAB);
  GIC_CHECK_ARG(B >= 1, "cider_pairwise: B=%d images", B);
  GIC_CHECK_ARG(n_keys >= 0, "cider_pairwise: n_keys=%lld", (long long)n_keys);
  GIC_CHECK_ARG(ld_ids >= L, "cider_pairwise: ld_ids=%lld below L=%d", (long long)ld_ids, L);
  GIC_CHECK_ARG(ids, "cider_pairwise: null ids");
  GIC_CHECK_ARG(lengths, "cider_pairwise: null lengths");
  GIC_CHECK_ARG(keys || n_keys == 0, "cider_pairwise: null keys");
  GIC_CHECK_ARG(idf || n_keys == 0, "cider_pairwise: null idf");
  GIC_CHECK_ARG(matrix || consensus || self_cider, "cider_pairwise: matrix, consensus and self_cider are all null");
  GIC_CHECK_ARG(std::isfinite(log_n) && log_n >= 0.f, "cider_pairwise: log_n must be finite and >= 0");
  PairArgs a{ids, (long)ld_ids, lengths, K, L, keys, idf, (long)n_keys, log_n, matrix, consensus, self_cider};
  hipLaunchKernelGGL(cider_pair_kernel, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, a);
  GIC_CHECK_LAUNCH("cider_pairwise");
  return GIC_OK;
}

}  // extern "C"
