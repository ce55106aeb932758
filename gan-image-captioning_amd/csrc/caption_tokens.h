// Caption tokens for the device-side metrics (cider.hip, cider_pair.hip, overlap.hip): a wave strips a caption's specials into LDS, a caption position
// is a lane, and every position packs the 4 tokens that start at it into one 64-bit window (15 bits per token).
#pragma once
#include "common.h"

namespace gic {

// orders a wave's LDS writes before the reads of its other lanes (one wave owns the buffer: no workgroup barrier needed)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A wave strips <PAD>/<S>/<E> from the first `len` ids of `row` into dst[0..count) (zeros after); returns count (wave-uniform).
// dst holds WAVE + 4 ints: the 4 past the end stay zero, so that window() of any position reads inside it.
__device__ __forceinline__ int strip_row(const int64_t* row, int len, int* dst) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t t = lane < len ? row[lane] : 0;
  const bool keep = lane < len && t > 2;
  const uint64_t bal = __ballot(keep);
  const int pos = __popcll(bal & ((1ull << lane) - 1ull));
  const int cnt = __popcll(bal);
  dst[lane] = 0;
  if (lane < 4) dst[WAVE + lane] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (keep) dst[pos] = (int)(t & 0x7fff);
  wave_lds_sync();
  return cnt;
}

// the 4 tokens from position p on, high to low, zero past the caption's end
__device__ __forceinline__ uint64_t window(const int* tok, int p) {
  return ((uint64_t)tok[p] << 45) | ((uint64_t)tok[p + 1] << 30) | ((uint64_t)tok[p + 2] << 15) | (uint64_t)tok[p + 3];
}

// ---------------------------------------------------------------- CIDEr-D (cider.hip, cider_pair.hip)
constexpr float kCiderTwoSigma2 = 2.f * 6.f * 6.f;      // sigma = 6

// the host table's key of the n-gram at a window's start: the window's first n tokens, tagged with n - 1 in bits 60..61
__device__ __forceinline__ uint64_t ngram_key(uint64_t win, int n) {
  const int drop = 15 * (4 - n);
  return ((uint64_t)(n - 1) << 60) | ((win >> drop) << drop);
}

// idf of a key: the table's value, or log N for an n-gram no document holds (df 0 -> log max(1, 0) = 0)
__device__ inline float lookup_idf(uint64_t key, const uint64_t* keys, const float* idf, long n_keys, float log_n) {
  long lo = 0, hi = n_keys;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n_keys && keys[lo] == key) ? idf[lo] : log_n;
}

}  // namespace gic
