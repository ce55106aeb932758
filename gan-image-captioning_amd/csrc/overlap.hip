// N-gram overlap metrics of token-id captions (gicap.h gic_caption_overlap): the per-candidate terms of corpus BLEU-1..4, the coco-caption
// ROUGE-L and an add-one smoothed sentence BLEU-4, next to CIDEr-D on the device.  DESIGN.md section 16.
//
// One workgroup (8 waves) per image; a caption position is a lane (lengths <= 64 = the wave width), as in cider.hip.
//   1. references   each wave strips one reference's specials by a ballot compaction into LDS (caption_tokens.h); then every position
//                   gets its 4-token window (15 bits per token, high to low, zero past the end).  The n-gram at a position is the top
//                   n tokens of its window: a stripped token is never 0, so two windows agree in their top n tokens at a position
//                   with a real n-gram only when both hold that n-gram.
//   2. candidates   one wave per candidate of the image.  Lane p owns the n-grams that start at p, n = 1..4 at once: one pass over the
//                   candidate's windows gives their counts and whether p is their first occurrence, one pass over each reference's
//                   windows the reference's counts; clipped_n = wave sum over first occurrences of min(count_c, max_r count_r).
//   3. LCS          per (candidate, reference) the bit-vector recurrence on one wave-uniform 64-bit word: lane j holds the reference's
//                   token j; for each candidate token, M = ballot(reference token == it), V <- (V + (V & M)) | (V & ~M); the LCS is the
//                   number of zero bits of V below the reference's length.  No O(L^2) table.
// Integer sums and a fixed-order loop over the references, no atomics: two calls give the same bits, in deterministic mode too.
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
constexpr int kStats = GIC_OVERLAP_STATS;
constexpr float kBeta2 = 1.2f * 1.2f;              // ROUGE-L: beta = 1.2
static_assert(kMaxLen == WAVE, "a caption position is a lane, and an LCS row is one 64-bit word");
static_assert(kStats == 10, "stats columns: clipped 1..4, total 1..4, length, closest reference length");

struct OverlapArgs {
  const int64_t* cand; long ldc; const int32_t* cand_len; const int32_t* cand_img; int n_cand, Lc;
  const int64_t* ref; long ldr; const int32_t* ref_len; const int32_t* ref_off; int n_ref, Lr, B, max_refs;
  int32_t* stats; float* rouge; float* sbleu;
};

// wave sum of ints, every lane gets it (an integer sum: the same bits in any order)
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// a candidate that is not scored: NaN scores, stats -1
__device__ __forceinline__ void mark_unscored(const OverlapArgs& a, int c) {
  for (int j = 0; j < kStats; ++j) a.stats[(long)c * kStats + j] = -1;
  a.rouge[c] = NAN;
  a.sbleu[c] = NAN;
}

__global__ __launch_bounds__(kThreads) void caption_overlap_kernel(const OverlapArgs a) {
  __shared__ int rtok[kMaxRefs][kMaxLen + 4];
  __shared__ uint64_t rwin[kMaxRefs][kMaxLen];
  __shared__ int rlen[kMaxRefs];
  __shared__ int ctok[kWaves][kMaxLen + 4];
  __shared__ uint64_t cwin[kWaves][kMaxLen];
  const int b = blockIdx.x, wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);

  if (b == 0)                                      // a candidate of no image in [0, B) is not scored
    for (int c = threadIdx.x; c < a.n_cand; c += kThreads)
      if (a.cand_img[c] < 0 || a.cand_img[c] >= a.B) mark_unscored(a, c);
  const int r0 = a.ref_off[b], r1 = a.ref_off[b + 1];
  const int R = r1 - r0;
  if (r0 < 0 || r1 > a.n_ref || R < 0 || R > a.max_refs) {     // offsets that break the contract: nothing read past them
    for (int c = threadIdx.x; c < a.n_cand; c += kThreads)
      if (a.cand_img[c] == b) mark_unscored(a, c);
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

  // 2. one wave per candidate of this image
  for (int c = wave; c < a.n_cand; c += kWaves) {
    if (a.cand_img[c] != b) continue;
    const int len = min(max(a.cand_len[c], 0), a.Lc);
    const int nc = strip_row(a.cand + (long)c * a.ldc, len, ctok[wave]);
    const int mytok = ctok[wave][lane];
    const uint64_t win = window(ctok[wave], lane);
    cwin[wave][lane] = win;
    wave_lds_sync();

    // the candidate's own counts of the n-grams at this lane, and whether an earlier position holds the same one
    int cc1 = 0, cc2 = 0, cc3 = 0, cc4 = 0, seen = 0;
    for (int q = 0; q < nc; ++q) {
      const uint64_t x = cwin[wave][q] ^ win;
      const int e1 = (x >> 45) == 0, e2 = (x >> 30) == 0, e3 = (x >> 15) == 0, e4 = x == 0;
      cc1 += e1; cc2 += e2; cc3 += e3; cc4 += e4;
      if (q < lane) seen |= e1 | (e2 << 1) | (e3 << 2) | (e4 << 3);
    }
    // per reference: its counts of them (the maximum over the references clips), its LCS with the candidate, its length
    int m1 = 0, m2 = 0, m3 = 0, m4 = 0;
    int lcs_p = 0;                                  // max_r lcs_r                 (precision = / nc)
    float rec = 0.f;                                // max_r lcs_r / len_r
    int close_key = 0x7fffffff;                     // min_r (|nc - len_r|, len_r) as |.| * 128 + len_r
    for (int r = 0; r < R; ++r) {
      const int lr = rlen[r];
      int c1 = 0, c2 = 0, c3 = 0, c4 = 0;
      for (int q = 0; q < lr; ++q) {
        const uint64_t x = rwin[r][q] ^ win;
        c1 += (x >> 45) == 0; c2 += (x >> 30) == 0; c3 += (x >> 15) == 0; c4 += x == 0;
      }
      m1 = max(m1, c1); m2 = max(m2, c2); m3 = max(m3, c3); m4 = max(m4, c4);
      close_key = min(close_key, abs(nc - lr) * 128 + lr);
      const int rt = rtok[r][lane];                 // 0 past the reference's end: no candidate token is 0
      uint64_t V = ~0ull;
      for (int i = 0; i < nc; ++i) {
        const uint64_t M = __ballot(rt == __builtin_amdgcn_readlane(mytok, i));
        V = (V + (V & M)) | (V & ~M);
      }
      const int lcs = __popcll(~V & (lr >= 64 ? ~0ull : (1ull << lr) - 1ull));
      lcs_p = max(lcs_p, lcs);
      if (lr > 0) rec = fmaxf(rec, (float)lcs / (float)lr);
    }
    // clipped counts: first occurrences only, the four orders in the four bytes of one wave sum
    int packed = 0;
    if (lane < nc && !(seen & 1)) packed |= min(cc1, m1);
    if (lane < nc - 1 && !(seen & 2)) packed |= min(cc2, m2) << 8;
    if (lane < nc - 2 && !(seen & 4)) packed |= min(cc3, m3) << 16;
    if (lane < nc - 3 && !(seen & 8)) packed |= min(cc4, m4) << 24;
    // a byte could carry past 255 only with > 255 clipped n-grams of one order; a caption has at most 64
    const unsigned clipped = (unsigned)wave_sum_i(packed);
    const int closest = close_key & 127;

    float rouge = 0.f, sb = 0.f;
    if (R > 0) {
      const float prec = nc > 0 ? (float)lcs_p / (float)nc : 0.f;
      if (prec > 0.f && rec > 0.f) rouge = (1.f + kBeta2) * prec * rec / (rec + kBeta2 * prec);
      const int k1 = (int)(clipped & 0xff);
      if (k1 > 0) {
        float lp = logf((float)k1 / (float)nc);
#pragma unroll
        for (int n = 2; n <= 4; ++n) {
          const int k = (int)((clipped >> (8 * (n - 1))) & 0xff), t = max(nc - n + 1, 0);
          lp += logf((float)(k + 1) / (float)(t + 1));
        }
        sb = expf(fminf(1.f - (float)closest / (float)nc, 0.f)) * expf(0.25f * lp);
      }
    }
    if (lane < kStats) {
      int v;
      if (lane < 4) v = (int)((clipped >> (8 * lane)) & 0xff);
      else if (lane < 8) v = max(nc - (lane - 4), 0);            // total_n = max(nc - n + 1, 0), n = lane - 3
      else v = lane == 8 ? nc : closest;
      a.stats[(long)c * kStats + lane] = R > 0 ? v : 0;
    }
    if (lane == 0) { a.rouge[c] = rouge; a.sbleu[c] = sb; }
  }
}

}  // namespace
}  // namespace gic

using namespace gic;

extern "C" {

int gic_caption_overlap(const int64_t* cand_ids, int64_t ld_cand, const int32_t* cand_len, const int32_t* cand_img, int32_t n_cand,
                        int32_t Lc, const int64_t* ref_ids, int64_t ld_ref, const int32_t* ref_len, const int32_t* ref_off, int32_t n_ref,
                        int32_t Lr, int32_t B, int32_t max_refs, int32_t V, int32_t* stats, float* rouge, float* sbleu, void* stream) {
  if (V > GIC_CIDER_MAX_VOCAB) { set_last_error("caption_overlap: V=%d > %d (15-bit n-gram windows)", V, GIC_CIDER_MAX_VOCAB); return GIC_ERR_UNSUPPORTED; }
  if (Lc > GIC_CIDER_MAX_LEN || Lr > GIC_CIDER_MAX_LEN) {
    set_last_error("caption_overlap: caption length Lc=%d / Lr=%d > %d", Lc, Lr, GIC_CIDER_MAX_LEN);
    return GIC_ERR_UNSUPPORTED;
  }
  if (max_refs > GIC_CIDER_MAX_REFS) {
    set_last_error("caption_overlap: %d references per image > %d", max_refs, GIC_CIDER_MAX_REFS);
    return GIC_ERR_UNSUPPORTED;
  }
  GIC_CHECK_ARG(V >= 1 && n_cand >= 0 && Lc >= 0 && n_ref >= 0 && Lr >= 0 && B >= 0 && max_refs >= 0,
                "caption_overlap: negative size or V < 1");
  GIC_CHECK_ARG(ld_cand >= Lc && ld_ref >= Lr, "caption_overlap: row stride below the row length");
  if (n_cand == 0) return GIC_OK;
  GIC_CHECK_ARG(B >= 1, "caption_overlap: candidates but no image");
  GIC_CHECK_ARG(cand_len && cand_img && stats && rouge && sbleu && ref_off && (cand_ids || Lc == 0), "caption_overlap: null pointer");
  GIC_CHECK_ARG((ref_ids && ref_len) || n_ref == 0 || Lr == 0, "caption_overlap: null reference pointer");
  GIC_CHECK_ARG(n_ref == 0 || ref_len, "caption_overlap: null reference lengths");
  OverlapArgs a{cand_ids, (long)ld_cand, cand_len, cand_img, n_cand, Lc, ref_ids, (long)ld_ref, ref_len, ref_off, n_ref, Lr, B, max_refs,
                stats, rouge, sbleu};
  hipLaunchKernelGGL(caption_overlap_kernel, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, a);
  GIC_CHECK_LAUNCH("caption_overlap");
  return GIC_OK;
}

}  // extern "C"
