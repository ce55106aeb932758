// Caption tokens for the device-side metrics (cider.hip, overlap.hip): a wave strips a caption's specials into LDS, a caption position
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

}  // namespace gic
