// Device helpers shared by the trunk's convolution kernels: the counted wait, 16-byte accesses through a buffer descriptor (with the one copy
// of the gfx950 store workaround), the DPP exchanges inside a row of 16 lanes, the LDS layout checks.  BatchNorm on load: bn_fold.h.
#pragma once
#include "common.h"
#include <initializer_list>

namespace gic {

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// 16-byte accesses through a buffer descriptor: per-lane byte offset + scalar byte offset
__device__ __forceinline__ u32x4 buf_load16(const __amdgpu_buffer_rsrc_t r, const int voff, const int soff) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
}
__device__ __forceinline__ void buf_store16(const u32x4 v, const __amdgpu_buffer_rsrc_t r, const int voff, const int soff) {
  // The tile offset rides in the per-lane offset, not in the scalar one: the compiler (hipcc 7.2) assumes a store of more than 8 bytes
  // with an SGPR offset needs no wait state before a VALU instruction overwrites its data registers and schedules one right behind
  // it; on gfx950 that instruction's result reached memory in place of the first dword (sporadically, lanes 12-15 of each row of 16).
#ifdef GIC_STORE_SOFF                                                      // (measurement build: the form that exposes the hazard)
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, soff, 0);
#else
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff + soff, 0, 0);
#endif
}

// Lane l's value of its neighbour l ^ X inside its row of 16 lanes, on the VALU (DPP: fused into the addition that consumes it).
// __shfl_xor is ds_bpermute_b32 -- an LDS instruction: 30 of them per reduce-scatter pair in four dependent stages, queued behind the
// weight fragment reads of all eight waves.
template <int CTRL>
__device__ __forceinline__ float row_dpp(const float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_xor4(const float v) {                                              // lanes with bit 2 clear read l + 4 (row_ror:12,
  const int x = __builtin_bit_cast(int, v);                                                             // banks 0 and 2), the others l - 4 (row_ror:4)
  int a = __builtin_amdgcn_update_dpp(0, x, 0x12C, 0xF, 0x5, false);
  a = __builtin_amdgcn_update_dpp(a, x, 0x124, 0xF, 0xA, false);
  return __builtin_bit_cast(float, a);
}

// Sum over the 16 lanes of a row (lr) of 16 per-lane values, value e ending up in lane lr == e: a reduce-scatter butterfly, 15 lane
// exchanges and 15 additions instead of 16 separate registers that live across the whole kernel.  (l ^ 8: row_ror:8; l ^ 2, l ^ 1: quad_perm)
__device__ __forceinline__ float row_reduce_scatter16(const float (&v)[16], const int lr) {
  float t[8], u[4], x[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) { const bool up = lr & 8; t[i] = (up ? v[i + 8] : v[i]) + row_dpp<0x128>(up ? v[i] : v[i + 8]); }
#pragma unroll
  for (int i = 0; i < 4; ++i) { const bool up = lr & 4; u[i] = (up ? t[i + 4] : t[i]) + row_xor4(up ? t[i] : t[i + 4]); }
#pragma unroll
  for (int i = 0; i < 2; ++i) { const bool up = lr & 2; x[i] = (up ? u[i + 2] : u[i]) + row_dpp<0x4E>(up ? u[i] : u[i + 2]); }
  const bool up = lr & 1;
  return (up ? x[1] : x[0]) + row_dpp<0xB1>(up ? x[0] : x[1]);
}

// A kernel's dynamic LDS image is written once, as a constexpr layout function beside the kernel: the kernel takes its offsets from it with its
// template arguments and asserts lds_ok on them, select_* takes the byte count from it with the plan's values.
constexpr int kLdsMax = 160 * 1024;
constexpr bool lds_ok(std::initializer_list<int> offsets, int bytes) {    // 16-byte pieces throughout, and the total fits a CU
  for (const int o : offsets) if (o % 16) return false;
  return bytes % 16 == 0 && bytes <= kLdsMax;
}

}  // namespace gic
