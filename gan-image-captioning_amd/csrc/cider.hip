// CIDEr-D scoring of token-id captions (gicap.h gic_cider_d): the coco-caption CiderScorer (Vedantam et al. 2015) on the device, so
// that SCST rewards and CIDEr-D evaluation never leave it.  DESIGN.md section 13.
//
// One workgroup (8 waves) per image; a caption position is a lane (lengths <= 64 = the wave width).
//   1. references   each wave strips one reference's specials (<PAD>, <S>, <E>) by a ballot compaction into LDS; then every position
//                   gets its 4-token window (15 bits per token, high to low, zero past the end): the n-gram key of position p is the
//                   window with the last 4 - n tokens cleared, tagged with n - 1 in bits 60..61 -- the host table's key format.
//   2. ref vectors  one wave per (reference, n): lane p owns the n-gram at p; it is the n-gram's first occurrence when no earlier
//                   position holds the same key, its count is the number of positions that do; first occurrences look their idf up by
//                   binary search in the global table (absent = df 0 = log N); norm_n = sqrt(wave sum of (count * idf)^2).
//   3. candidates   one wave per candidate of the image: the same first-occurrence / count / idf per lane, the candidate's counts from
//                   64-bit shuffles, the reference counts from the LDS windows; sim_n(c, r) = wave sum over first occurrences of
//                   min(vc, vr) * vr, over the norms, times the bigram-length penalty.  score = 10 * mean_n(sum_r sim_n) / |R|.
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
constexpr int kMaxRefs = GIC_CIDER_MAX_REFS;
constexpr float kTwoSigma2 = kCiderTwoSigma2;
static_assert(kMaxLen == WAVE, "a caption position is a lane");

struct CiderArgs {
  const int64_t* cand; long ldc; const int32_t* cand_len; const int32_t* cand_img; int n_cand, Lc;
  const int64_t* ref; long ldr; const int32_t* ref_len; const int32_t* ref_off; int n_ref, Lr, B, max_refs;
  const uint64_t* keys; const float* idf; long K; float log_n;
  float* scores;
};

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, WAVE), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, WAVE);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ float lookup_idf(uint64_t key, const CiderArgs& a) { return gic::lookup_idf(key, a.keys, a.idf, a.K, a.log_n); }

__global__ __launch_bounds__(kThreads) void cider_d_kernel(const CiderArgs a) {
  __shared__ int rtok[kMaxRefs][kMaxLen + 4];
  __shared__ uint64_t rwin[kMaxRefs][kMaxLen];
  __shared__ float rnorm[kMaxRefs][4];
  __shared__ int rlen[kMaxRefs];
  __shared__ int ctok[kWaves][kMaxLen + 4];
  const int b = blockIdx.x, wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);

  if (b == 0)                                      // a candidate of no image in [0, B) is not scored: NaN
    for (int c = threadIdx.x; c < a.n_cand; c += kThreads)
      if (a.cand_img[c] < 0 || a.cand_img[c] >= a.B) a.scores[c] = NAN;
  const int r0 = a.ref_off[b], r1 = a.ref_off[b + 1];
  const int R = r1 - r0;
  if (r0 < 0 || r1 > a.n_ref || R < 0 || R > a.max_refs) {     // offsets that break the contract: NaN, nothing read past them
    for (int c = threadIdx.x; c < a.n_cand; c += kThreads)
      if (a.cand_img[c] == b) a.scores[c] = NAN;
    return;
  }

  // 1. references: stripped tokens, then the 4-token window of every position
  for (int r = wave; r < R; r += kWaves) {
    const int len = min(max(a.ref_len[r0 + r], 0), a.Lr);
    const int cnt = strip_row(a.ref + (long)(r0 + r) * a.ldr, len, rtok[r]);
    if (lane == 0) rlen[r] = cnt;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < R * kMaxLen; i += kThreads) rwin[i / kMaxLen][i % kMaxLen] = window(rtok[i / kMaxLen], i % kMaxLen);
  __syncthreads();

  // 2. per (reference, n): the norm of its idf-weighted count vector
  for (int task = wave; task < 4 * R; task += kWaves) {
    const int r = task >> 2, n = (task & 3) + 1, m = rlen[r] - n + 1;          // m = the reference's number of n-grams
    float v2 = 0.f;
    if (lane < m) {
      const uint64_t key = ngram_key(rwin[r][lane], n);
      int cnt = 0;
      bool first = true;
      for (int q = 0; q < m; ++q)
        if (ngram_key(rwin[r][q], n) == key) { ++cnt; first = first && q >= lane; }
      if (first) {
        const float v = (float)cnt * lookup_idf(key, a);
        v2 = v * v;
      }
    }
    v2 = wave_sum(v2);
    if (lane == 0) rnorm[r][n - 1] = sqrtf(v2);
  }
  __syncthreads();

  // 3. one wave per candidate of this image
  for (int c = wave; c < a.n_cand; c += kWaves) {
    if (a.cand_img[c] != b) continue;
    const int len = min(max(a.cand_len[c], 0), a.Lc);
    const int nc = strip_row(a.cand + (long)c * a.ldc, len, ctok[wave]);
    const uint64_t win = window(ctok[wave], lane);
    const int lc2 = max(nc - 1, 0);                                             // "length" = the number of bigrams
    float acc = 0.f;
    for (int n = 1; n <= 4; ++n) {
      const int m = nc - n + 1;
      const uint64_t key = ngram_key(win, n);
      int cnt = 0;
      bool first = true;
      for (int q = 0; q < m; ++q) {                                             // every lane shuffles: m is wave-uniform
        if (shfl64(key, q) == key) { ++cnt; first = first && q >= lane; }
      }
      const bool own = lane < m && first;
      const float idf = own ? lookup_idf(key, a) : 0.f;
      const float vc = (float)cnt * idf;
      const float norm_c = sqrtf(wave_sum(own ? vc * vc : 0.f));
      float sum_r = 0.f;
      for (int r = 0; r < R; ++r) {
        const int mr = rlen[r] - n + 1;
        int cr = 0;
        if (own)
          for (int q = 0; q < mr; ++q) cr += ngram_key(rwin[r][q], n) == key;
        const float vr = (float)cr * idf;
        float val = wave_sum(own ? fminf(vc, vr) * vr : 0.f);
        const float norm_r = rnorm[r][n - 1];
        if (norm_c != 0.f && norm_r != 0.f) val /= norm_c * norm_r;
        const float delta = (float)(lc2 - max(rlen[r] - 1, 0));
        sum_r += val * expf(-(delta * delta) / kTwoSigma2);
      }
      acc += sum_r;
    }
    if (lane == 0) a.scores[c] = R > 0 ? acc / 4.f / (float)R * 10.f : 0.f;
  }
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" {

int gic_cider_d(const int64_t* cand_ids, int64_t ld_cand, const int32_t* cand_len, const int32_t* cand_img, int32_t n_cand, int32_t Lc,
                const int64_t* ref_ids, int64_t ld_ref, const int32_t* ref_len, const int32_t* ref_off, int32_t n_ref, int32_t Lr,
                int32_t B, int32_t max_refs, const uint64_t* keys, const float* idf, int64_t K, float log_n, int32_t V, float* scores,
                void* stream) {
  if (V > GIC_CIDER_MAX_VOCAB) { set_last_error("cider_d: V=%d > %d (15-bit n-gram keys)", V, GIC_CIDER_MAX_VOCAB); return GIC_ERR_UNSUPPORTED; }
  if (Lc > GIC_CIDER_MAX_LEN || Lr > GIC_CIDER_MAX_LEN) {
    set_last_error("cider_d: caption length Lc=%d / Lr=%d > %d", Lc, Lr, GIC_CIDER_MAX_LEN);
    return GIC_ERR_UNSUPPORTED;
  }
  if (max_refs > GIC_CIDER_MAX_REFS) { set_last_error("cider_d: %d references per image > %d", max_refs, GIC_CIDER_MAX_REFS); return GIC_ERR_UNSUPPORTED; }
  GIC_CHECK_ARG(V >= 1 && n_cand >= 0 && Lc >= 0 && n_ref >= 0 && Lr >= 0 && B >= 0 && max_refs >= 0 && K >= 0,
                "cider_d: negative size or V < 1");
  GIC_CHECK_ARG(ld_cand >= Lc && ld_ref >= Lr, "cider_d: row stride below the row length");
  GIC_CHECK_ARG(std::isfinite(log_n) && log_n >= 0.f, "cider_d: log_n must be finite and >= 0");
  if (n_cand == 0) return GIC_OK;
  GIC_CHECK_ARG(B >= 1, "cider_d: candidates but no image");
  GIC_CHECK_ARG(cand_len && cand_img && scores && ref_off && (cand_ids || Lc == 0), "cider_d: null pointer");
  GIC_CHECK_ARG((ref_ids && ref_len) || n_ref == 0 || Lr == 0, "cider_d: null reference pointer");
  GIC_CHECK_ARG(n_ref == 0 || ref_len, "cider_d: null reference lengths");
  GIC_CHECK_ARG((keys && idf) || K == 0, "cider_d: null table");
  CiderArgs a{cand_ids, (long)ld_cand, cand_len, cand_img, n_cand, Lc, ref_ids, (long)ld_ref, ref_len, ref_off, n_ref, Lr, B, max_refs,
              keys, idf, (long)K, log_n, scores};
  hipLaunchKernelGGL(cider_d_kernel, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, a);
  GIC_CHECK_LAUNCH("cider_d");
  return GIC_OK;
}

}  // extern "C"
