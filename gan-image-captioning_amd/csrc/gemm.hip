// MFMA GEMM family for gfx950 (MI355X): every dense contraction on the hot path (trunk convolutions as implicit GEMM, LSTM
// gates, vocab projection, discriminator embedding / highway / head, all dgrad and wgrad products, the encoder head).
//
// Two kernels:
//   gemm_kernel   4 waves (2x2), 128x128 or 64x64 tile.  Any operand layout (k-contiguous: LDS image [row][k], ds_read_b128
//                 fragments; m/n-contiguous: LDS image [k][row], bf16 fragments out of ds_read_b64_tr_b16, so dgrad / wgrad
//                 need no transposed copies in HBM), bf16 (v_mfma_f32_16x16x32_bf16) or exact f32 (v_mfma_f32_16x16x4_f32,
//                 parity mode), register-staged double buffer or 3-stage LDS-DMA ring, split-K over gridDim.y (f32 atomics)
//                 for skinny / deep-K products, highway epilogue, 16-byte accesses when shapes allow, scalar fallback.
//                 The vectorised weight-gradient form (both operands row-major over K) has a second instantiation, EPI_WGRAD: the
//                 column sums of A (the layer's bias gradient) out of the staged A chunks of the first N tile's workgroups, and a
//                 second output matrix from column n_split on (gemm.h).
//   tile8_kernel  8 waves (4x2), 128x128 or 128x64 tile, bf16 k-contiguous operands only: buffer-descriptor LDS-DMA ring of 1 /
//                 2 / 4 stages.  Every trunk convolution in bf16 mode and the wide plain / highway products (highway: row-padded
//                 bf16 buffers only, select_tile8's highway_wide; every other highway product is gemm_kernel's).  See its header.
// Both: XCD-aware block -> tile map (xcd_run: each of the 8 XCDs owns a contiguous run of tiles that share B panels in its L2), C
// tile staged through LDS for 16-byte row stores, BatchNorm column sums folded across the block in the epilogue.
// What the two share with each other and with the dynamic-LDS convolution kernels is in gemm_device.h (the LDS swizzle, the MFMA
// block, the highway gate and keep draw, the convolution addressing); gemm_kernel's LDS image of an operand (its stores and fragment
// reads) is written once (g4_*) and applied to A and to B.  The staged-C epilogues, gemm_kernel's `gload` and tile8's whole-tile `compute`
// are each kernel's own text: DESIGN.md section 4.
#include "gemm.h"
#include "conv3x3.h"
#include "conv1x1_stream.h"
#include "conv1x1_panel.h"
#include "conv1x1_pix.h"
#include "conv_stem.h"
#include "bn_fold.h"
#include "gemm_device.h"
#include "kernels.h"

#include <stdlib.h>
#include <string.h>
#include <atomic>

namespace gic {

namespace {

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef const __attribute__((address_space(1))) u32x4* gptr_u4;

// 16 zero bytes in global memory: the source of an LDS-DMA chunk that falls outside the operand (conv padding, M/K tails)
__device__ __attribute__((aligned(16))) unsigned int g_zero16[4] = {0u, 0u, 0u, 0u};
typedef const __attribute__((address_space(1))) void* gbl_void_ptr;

#ifdef GIC_STAMPS
}  // anon
__device__ unsigned long long g_stamp[32];
namespace {
#define STAMP(i) do { if (tid == 0 && blockIdx.y == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1)) { \
  const int o_ = blockIdx.x == 0 ? 0 : 16; g_stamp[o_ + 2 * (i)] = __builtin_amdgcn_s_memtime(); g_stamp[o_ + 2 * (i) + 1] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#define DBG d.dbg      // phase ablation (tools/gemm_stamps.py): 1 = no DMA after the prologue, 2 = no MFMA phase
#else
#define STAMP(i) do {} while (0)
#define DBG 0
#endif

template <typename T> struct GlobalPtr { typedef const __attribute__((address_space(1))) T* type; };

// ---- gemm_kernel's handling of ONE operand of a K tile, applied to A (rows m, BR = BM) and to B (rows n, BR = BN).  KC: k-contiguous
// (LDS image [row][k]) or row-contiguous ([k][row]); S: the LDS row stride in bytes; 256 threads, chunk c = tid + 256 i.
// Arguments, in this order wherever they occur: the LDS image; the operand (P, ld); its rows (row0 = the tile's first, R = the operand's
// count); the K tile (k0 = its first k, K = the operand's depth); the thread (tid, or lr = lane & 15, lg = lane >> 4).
// registers -> LDS image
template <typename TI, bool KC, int BR, int S, int NC>
__device__ __forceinline__ void g4_store(unsigned char* img, const u32x4 (&reg)[NC], const int tid) {
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = tid + i * 256;
    if constexpr (KC) {
      *(u32x4*)(img + (c >> 3) * S + (c & 7) * 16) = reg[i];
    } else {
      constexpr int CPR = BR / (16 / (int)sizeof(TI));
      *(u32x4*)(img + (c / CPR) * S + (c % CPR) * 16) = reg[i];
    }
  }
}
// global -> LDS image, element by element (scalar fallback: unaligned operands)
template <typename TI, bool KC, int BR, int S>
__device__ __forceinline__ void g4_store_scalar(unsigned char* img, const typename GlobalPtr<TI>::type P, const long ld, const int row0,
                                                const int R, const int k0, const int K, const int tid) {
  constexpr int SZ = sizeof(TI), BK = 128 / SZ;
  for (int e = tid; e < BR * BK; e += 256) {
    TI v = (TI)0.f;
    if constexpr (KC) {
      const int row = e / BK, kk = e % BK;
      const int r = row0 + row, k = k0 + kk;
      if (r < R && k < K) v = P[(long)r * ld + k];
      *(TI*)(img + row * S + kk * SZ) = v;
    } else {
      const int kk = e / BR, row = e % BR;
      const int r = row0 + row, k = k0 + kk;
      if (r < R && k < K) v = P[(long)k * ld + r];
      *(TI*)(img + kk * S + row * SZ) = v;
    }
  }
}
// LDS image -> the bf16 fragment of rows r0 .. r0 + 15 for the 32-deep K step ks
template <bool KC, bool PIPE, int S>
__device__ __forceinline__ bf16x8 g4_frag_bf16(const unsigned char* img, const int r0, const int ks, const int lr, const int lg) {
  if constexpr (PIPE) {
    return *(const bf16x8*)(img + (r0 + lr) * 128 + swz_chunk(r0 + lr, ks * 4 + lg));
  } else if constexpr (KC) {
    return *(const bf16x8*)(img + (r0 + lr) * S + ks * 64 + lg * 16);
  } else {
    // [k][row] image: lane (q=lr>>2, p=lr&3) addresses row k0+q, cols 4p..4p+3; receives column lr
    const unsigned char* p0 = img + (ks * 32 + lg * 8 + (lr >> 2)) * S + (r0 + 4 * (lr & 3)) * 2;
    const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p0);
    const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p0 + 4 * S));
    return __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
  }
}
// ... and the f32 one: lane group lg owns k = 8*lg .. 8*lg+7 of the 32-wide tile
template <bool KC, bool PIPE, int S>
__device__ __forceinline__ void g4_frag_f32(float (&f)[8], const unsigned char* img, const int r0, const int lr, const int lg) {
  if constexpr (KC) {
    const int row = r0 + lr;
    const float4 v0 = *(const float4*)(img + row * S + (PIPE ? swz_chunk(row, 2 * lg) : 2 * lg * 16));
    const float4 v1 = *(const float4*)(img + row * S + (PIPE ? swz_chunk(row, 2 * lg + 1) : (2 * lg + 1) * 16));
    f[0] = v0.x; f[1] = v0.y; f[2] = v0.z; f[3] = v0.w;
    f[4] = v1.x; f[5] = v1.y; f[6] = v1.z; f[7] = v1.w;
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s) f[s] = *(const float*)(img + (lg * 8 + s) * S + (r0 + lr) * 4);
  }
}

// launches of the EPI_WGRAD form since the library was loaded, and those of them with a second output matrix (wgrad_launch_counts)
std::atomic<long> g_wgrad_launches{0}, g_wgrad_two{0};

// gemm_kernel's EPI argument for EPI_PLAIN with the weight-gradient extras of gemm.h (a_sum / a_sum2, C2 / n_split): never a descriptor's
// epi, chosen by the launch (Gemm4Plan.wg) for the <AKC = false, BKC = false, VEC> form alone, so that every other instantiation keeps its
// name and its code
constexpr int EPI_WGRAD = 4;

// one staged 16-byte chunk of an m-contiguous bf16 A (eight consecutive m of one k) added onto the thread's eight partial sums
__device__ __forceinline__ void g4_chunk_add(float (&s)[8], const u32x4 r) {
  const bf16x8 v = __builtin_bit_cast(bf16x8, r);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
}

// PIPE (k-contiguous, vectorised operands only): tiles reach LDS by LDS-DMA (global_load_lds, 16 B per lane, no VGPR
// staging) into a 3-stage ring; the loads of tile k+2 are in flight under the MFMAs of tiles k and k+1 behind a COUNTED
// s_waitcnt vmcnt and one raw s_barrier per K tile.  The LDS image is lane-linear per wave-instruction (128-byte rows, no
// padding), so the bank-conflict fix is an XOR of the 16-byte chunk index with (row>>1)&7, applied to the per-lane SOURCE
// address on the way in and to the ds_read_b128 address on the way out.
template <typename TI, typename TO, bool AKC, bool BKC, int BM, int BN, bool VEC, int EPI, bool CONV, bool PIPE>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmDesc d, const int k_tiles_per_split) {
  static_assert(!CONV || (AKC && BKC && VEC), "the implicit-GEMM convolution loader is k-contiguous and vectorised");
  static_assert(!PIPE || (AKC && BKC && VEC), "the LDS-DMA pipeline needs k-contiguous 16-byte chunks");
  constexpr bool WG = EPI == EPI_WGRAD;
  static_assert(!WG || (!AKC && !BKC && VEC && !CONV && !PIPE && sizeof(TI) == 2), "the weight-gradient extras exist in the vectorised m/n-contiguous bf16 form only");
  constexpr int SZ = sizeof(TI);
  constexpr int BK = 128 / SZ;          // K elements per tile
  constexpr int VE = 16 / SZ;           // elements per 16-byte chunk
  constexpr int SA = PIPE ? 128 : (AKC ? 144 : BM * SZ + 16);   // LDS row stride (bytes)
  constexpr int SB = PIPE ? 128 : (BKC ? 144 : BN * SZ + 16);
  constexpr int NSTAGE = PIPE ? 3 : 2;
  constexpr int A_BYTES = AKC ? BM * SA : BK * SA;
  constexpr int B_BYTES = BKC ? BN * SB : BK * SB;
  constexpr int BUF_BYTES = A_BYTES + B_BYTES;
  constexpr int TM = BM / 32, TN = BN / 32;      // 16x16 tiles per wave
  constexpr int CA = BM / 32, CB = BN / 32;      // 16-B chunks per thread per tile
  constexpr bool IS_BF16 = (SZ == 2);
  typedef typename GlobalPtr<TI>::type gptr_t;

  constexpr int EPI_BYTES = BM * (BN * (int)sizeof(TO) + 16) + 4 * (BN / 2) * 2 * 4;   // staged C tile + stats scratch
  constexpr int SMEM_BYTES = NSTAGE * BUF_BYTES > EPI_BYTES ? NSTAGE * BUF_BYTES : EPI_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  STAMP(0);
  const int wr = w >> 1, wc = w & 1;
  const int lr = lane & 15, lg = lane >> 4;

  // ---- XCD-aware tile assignment (bijective remap; blocks b and b+8 share an XCD)
  const int tiles_m = (d.M + BM - 1) / BM;
  const int bid = xcd_run(blockIdx.x, gridDim.x);
  const int bm0 = (bid % tiles_m) * BM;
  const int bn0 = (bid / tiles_m) * BN;

  gptr_t A = (gptr_t)d.A;
  gptr_t B = (gptr_t)d.B;
  const int M = d.M, N = d.N, K = d.K;
  const long lda = d.lda, ldb = d.ldb;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  u32x4 ra[CA], rb[CB];

  // ---- WG: column sums of A.  A thread's chunks all cover the same VE rows m (256 is a multiple of the BM / VE chunks of a k row), so it
  // keeps VE partial sums over the k it stages; the workgroups of the first N tile do (every m belongs to exactly one of them per split)
  float asum[WG ? VE : 1];
  bool asum_on = false;
  if constexpr (WG) {
    asum_on = d.a_sum && bn0 == 0;
#pragma unroll
    for (int e = 0; e < VE; ++e) asum[e] = 0.f;
  }

  // ---- implicit-GEMM convolution: per staged row (fixed per thread) the image and the top-left input pixel;
  // per thread ONE running (r, s, c) decomposition of its k (all of a thread's chunks share kc = tid & 7).
  long cv_base[CONV ? CA : 1];
  int cv_hi0[CONV ? CA : 1], cv_wi0[CONV ? CA : 1];
  int cv_r = 0, cv_s = 0, cv_c = 0;
  if constexpr (CONV) {
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int m = bm0 + ((tid + i * 256) >> 3);
      const ConvOrigin<long> o = conv_origin<long>(m, m < M, d.cHo, d.cWo, d.cH, d.cW, d.cStride, d.cPad);
      cv_hi0[i] = o.hi0; cv_wi0[i] = o.wi0; cv_base[i] = o.pix;
    }
    // PIPE: physical chunk slot tid&7 holds logical chunk (tid&7) ^ swizzle(row); the swizzle (row>>1)&7 is the same
    // for all of a thread's rows (they are 32 apart), so the thread still owns ONE k chunk per tile.
    const int kchunk = PIPE ? swz_dma_chunk(tid) : (tid & 7);
    const int k = blockIdx.y * k_tiles_per_split * BK + kchunk * VE;
    cv_c = k % d.cCin;
    const int t = k / d.cCin;
    cv_s = t % d.cKW;
    cv_r = t / d.cKW;
  }

  // global -> registers (VEC path).  Typed address_space(1) loads: a `cond ? *p : zero` on a generic pointer
  // makes the compiler select between the global address and a private zero and spill the staging registers.
  auto gload = [&](int kt) {
    if constexpr (VEC) {
      const int k0 = kt * BK;
      if constexpr (CONV) {
#pragma unroll
        for (int i = 0; i < CA; ++i) {
          ra[i] = (u32x4){0u, 0u, 0u, 0u};
          const int hi = cv_hi0[i] + cv_r, wi = cv_wi0[i] + cv_s;
          if (cv_r < d.cKH && hi >= 0 && hi < d.cH && wi >= 0 && wi < d.cW)
            ra[i] = *(gptr_u4)(A + (cv_base[i] + (long)cv_r * d.cW + cv_s) * d.cCin + cv_c);
        }
      } else {
#pragma unroll
        for (int i = 0; i < CA; ++i) {
          const int c = tid + i * 256;
          ra[i] = (u32x4){0u, 0u, 0u, 0u};
          if constexpr (AKC) {
            const int m = bm0 + (c >> 3), k = k0 + (c & 7) * VE;
            if (m < M && k < K) ra[i] = *(gptr_u4)(A + (long)m * lda + k);
          } else {
            constexpr int CPR = BM / VE;
            const int k = k0 + c / CPR, m = bm0 + (c % CPR) * VE;
            if (k < K && m < M) ra[i] = *(gptr_u4)(A + (long)k * lda + m);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < CB; ++i) {
        const int c = tid + i * 256;
        rb[i] = (u32x4){0u, 0u, 0u, 0u};
        if constexpr (BKC) {
          const int n = bn0 + (c >> 3), k = k0 + (c & 7) * VE;
          if (n < N && k < K) rb[i] = *(gptr_u4)(B + (long)n * ldb + k);
        } else {
          constexpr int CPR = BN / VE;
          const int k = k0 + c / CPR, n = bn0 + (c % CPR) * VE;
          if (k < K && n < N) rb[i] = *(gptr_u4)(B + (long)k * ldb + n);
        }
      }
      if constexpr (CONV) conv_tap_advance(cv_r, cv_s, cv_c, BK, d.cCin, d.cKW);
    }
  };

  // registers (VEC) or global (scalar fallback) -> LDS buffer `buf`
  auto sstore = [&](int kt, int buf) {
    unsigned char* sA = smem + buf * BUF_BYTES;
    unsigned char* sB = sA + A_BYTES;
    if constexpr (VEC) {
      if constexpr (WG) {
        if (asum_on) {                                   // (zero-filled tail chunks add zero)
#pragma unroll
          for (int i = 0; i < CA; ++i) g4_chunk_add(asum, ra[i]);
        }
      }
      g4_store<TI, AKC, BM, SA>(sA, ra, tid);
      g4_store<TI, BKC, BN, SB>(sB, rb, tid);
    } else {
      g4_store_scalar<TI, AKC, BM, SA>(sA, A, lda, bm0, M, kt * BK, K, tid);
      g4_store_scalar<TI, BKC, BN, SB>(sB, B, ldb, bn0, N, kt * BK, K, tid);
    }
  };

  // ---- PIPE: one K tile -> LDS stage `buf` by LDS-DMA.  Chunk c = tid + i*256 lands at byte 16*c of the stage's A (B)
  // image: the wave-instruction's 64 lanes write 1 KiB contiguously (wave-uniform base + lane*16).
  auto issue = [&](int kt, int buf) {
    if constexpr (PIPE) {
      unsigned char* sA = smem + buf * BUF_BYTES;
      unsigned char* sB = sA + A_BYTES;
      const int k0 = kt * BK;
      const int kc = swz_dma_chunk(tid) * VE;                     // logical k offset of this thread's chunk
      const int wbase = (tid & ~63) * 16;
#pragma unroll
      for (int i = 0; i < CA; ++i) {
        const int c = tid + i * 256;
        const TI* src = (const TI*)g_zero16;
        if constexpr (CONV) {
          const int hi = cv_hi0[i] + cv_r, wi = cv_wi0[i] + cv_s;
          if (cv_r < d.cKH && hi >= 0 && hi < d.cH && wi >= 0 && wi < d.cW)
            src = (const TI*)d.A + (cv_base[i] + (long)cv_r * d.cW + cv_s) * d.cCin + cv_c;
        } else {
          const int m = bm0 + (c >> 3), k = k0 + kc;
          if (m < M && k < K) src = (const TI*)d.A + (long)m * lda + k;
        }
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(sA + i * 4096 + wbase), 16, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < CB; ++i) {
        const int c = tid + i * 256;
        const TI* src = (const TI*)g_zero16;
        const int n = bn0 + (c >> 3), k = k0 + kc;
        if (n < N && k < K) src = (const TI*)d.B + (long)n * ldb + k;
        __builtin_amdgcn_global_load_lds((gbl_void_ptr)src, (lds_void_ptr)(sB + i * 4096 + wbase), 16, 0, 0);
      }
      if constexpr (CONV) conv_tap_advance(cv_r, cv_s, cv_c, BK, d.cCin, d.cKW);
    }
  };

  auto compute = [&](int buf) {
    const unsigned char* sA = smem + buf * BUF_BYTES;
    const unsigned char* sB = sA + A_BYTES;
    if constexpr (IS_BF16) {
#pragma unroll
      for (int ks = 0; ks < BK / 32; ++ks) {
        bf16x8 fa[TM], fb[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) fa[t] = g4_frag_bf16<AKC, PIPE, SA>(sA, wr * (BM / 2) + t * 16, ks, lr, lg);
#pragma unroll
        for (int t = 0; t < TN; ++t) fb[t] = g4_frag_bf16<BKC, PIPE, SB>(sB, wc * (BN / 2) + t * 16, ks, lr, lg);
        mfma_block(acc, fa, fb);
      }
    } else {
      // f32: MFMA step s contracts k in {8g+s : g=0..3} (same map for A and B, so the sum covers all 32).
      float fa[TM][8], fb[TN][8];
#pragma unroll
      for (int t = 0; t < TM; ++t) g4_frag_f32<AKC, PIPE, SA>(fa[t], sA, wr * (BM / 2) + t * 16, lr, lg);
#pragma unroll
      for (int t = 0; t < TN; ++t) g4_frag_f32<BKC, PIPE, SB>(fb[t], sB, wc * (BN / 2) + t * 16, lr, lg);
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
    }
  };

  // ---- K loop over this block's split: [kt0, kt1)
  const int nk = (K + BK - 1) / BK;
  const int kt0 = blockIdx.y * k_tiles_per_split;
  const int kt1 = min(nk, kt0 + k_tiles_per_split);
  if constexpr (PIPE) {
    if (kt0 < kt1) {
      constexpr int NL = CA + CB;                       // LDS-DMA instructions per thread per stage
      STAMP(1);
      issue(kt0, 0);
      if (kt0 + 1 < kt1) issue(kt0 + 1, 1);
      int buf = 0;
      for (int kt = kt0; kt < kt1; ++kt) {
        // stage kt has landed once all but this wave's newest NL DMAs (stage kt+1) are done; the barrier then
        // publishes every wave's part of it and retires all reads of the stage that is about to be refilled.
        if (kt + 1 < kt1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt == kt0) STAMP(2);
        if (kt + 2 < kt1 && !(DBG & 1)) issue(kt + 2, buf >= 1 ? buf - 1 : 2);      // (buf + 2) % 3
        if (!(DBG & 2)) compute(buf);
        buf = buf == 2 ? 0 : buf + 1;
      }
      __syncthreads();                                  // all fragment reads done before the epilogue reuses LDS
      STAMP(3);
    }
  } else if (kt0 < kt1) {
    int cur = 0;
    gload(kt0);
    sstore(kt0, 0);
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
      const bool more = kt + 1 < kt1;
      if (more) gload(kt + 1);          // next tile's HBM/L2 loads fly under this tile's MFMAs
      compute(cur);
      if (more) sstore(kt + 1, cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }

  // ---- epilogue.  C/D map: col = lane&15, row = (lane>>4)*4 + reg
  TO* __restrict__ C = (TO*)d.C;
  long ldc = d.ldc;
#define LDC (WG ? ldc : d.ldc)      /* every other instantiation reads the descriptor where it always did: its instruction stream is unchanged */
  const bool split = gridDim.y > 1;

  if constexpr (WG) {
    // the tiles from column n_split on belong to C2 (n_split is a multiple of BN: a tile has one destination)
    if (d.C2 && bn0 >= d.n_split) { C = (TO*)d.C2 - d.n_split; ldc = d.ldc2; }
    if (asum_on) {                                       // block-uniform
      // fold the partials of the 256 / CPR threads that share an m chunk through the epilogue's LDS area (the K loop's last barrier has
      // retired the ring), in a fixed order; then one store, += or (split-K) atomicAdd per m
      constexpr int CPR = BM / VE, G = 256 / CPR;
      static_assert(G * BM * 4 <= SMEM_BYTES, "the column-sum partials must fit the LDS allocation");
      float* sS = (float*)smem;                          // [G][BM]
#pragma unroll
      for (int e = 0; e < VE; ++e) sS[(tid / CPR) * BM + (tid % CPR) * VE + e] = asum[e];
      __syncthreads();
      if (tid < BM && bm0 + tid < M) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) t += sS[g * BM + tid];
        const int m = bm0 + tid;
        if (split) {
          atomicAdd(d.a_sum + m, t);
          if (d.a_sum2) atomicAdd(d.a_sum2 + m, t);
        } else {
          d.a_sum[m] = d.accumulate ? d.a_sum[m] + t : t;
          if (d.a_sum2) d.a_sum2[m] = d.accumulate ? d.a_sum2[m] + t : t;
        }
      }
      __syncthreads();                                   // the C tile is staged over this area
    }
  }

  // Staged path (conv / plain products that overwrite C): the tile goes through LDS so that every global store
  // is a 16-byte piece of a contiguous output row (a direct store of the MFMA layout writes 32-byte row
  // fragments, 2 bytes per lane), and the BatchNorm column sums are folded across the block before ONE atomic
  // per column lands in one of `stats_nrep` replicas (few adders per address: global f32 atomics serialise).
  if constexpr (EPI != EPI_HIGHWAY) {
    constexpr int OSZ = sizeof(TO);
    constexpr int OVE = 16 / OSZ;
    constexpr int SC = BN * OSZ + 16;                       // LDS row stride of the C tile
    static_assert(BM * SC + 4 * (BN / 2) * 2 * 4 <= SMEM_BYTES, "C tile + stats scratch must fit the LDS allocation");
    const bool staged = !split && !d.accumulate && (N % OVE == 0) && (LDC % OVE == 0) && ((((uintptr_t)(WG ? (const void*)C : (const void*)d.C)) & 15) == 0);
    if (staged) {
      unsigned char* sC = smem;
      float* sStat = (float*)(smem + BM * SC);               // [4 waves][BN/2][2]
      float st_s[TN], st_q[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int nl = wc * (BN / 2) + j * 16 + lr;
        const int n = bn0 + nl;
        const float bias = (d.bias && n < N) ? d.bias[n] : 0.f;
        st_s[j] = 0.f; st_q[j] = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ml = wr * (BM / 2) + i * 16 + lg * 4 + r;
            const float v = d.alpha * acc[i][j][r] + bias;
            *(TO*)(sC + ml * SC + nl * OSZ) = from_f32<TO>(v);
            if (EPI == EPI_BNSTATS && bm0 + ml < M) { st_s[j] += v; st_q[j] += v * v; }
          }
        }
        if constexpr (EPI == EPI_BNSTATS) {
          st_s[j] += __shfl_xor(st_s[j], 16, 64); st_q[j] += __shfl_xor(st_q[j], 16, 64);
          st_s[j] += __shfl_xor(st_s[j], 32, 64); st_q[j] += __shfl_xor(st_q[j], 32, 64);
          if (lg == 0) { sStat[(w * (BN / 2) + j * 16 + lr) * 2] = st_s[j]; sStat[(w * (BN / 2) + j * 16 + lr) * 2 + 1] = st_q[j]; }
        }
      }
      __syncthreads();
      STAMP(4);
      if constexpr (EPI == EPI_BNSTATS) {
        if (tid < BN) {                                        // column tid: waves (wr=0, wc) and (wr=1, wc)
          const int cwc = tid / (BN / 2), cl = tid % (BN / 2), n = bn0 + tid;
          if (n < N) {
            const float s0 = sStat[((0 * 2 + cwc) * (BN / 2) + cl) * 2] + sStat[((1 * 2 + cwc) * (BN / 2) + cl) * 2];
            const float q0 = sStat[((0 * 2 + cwc) * (BN / 2) + cl) * 2 + 1] + sStat[((1 * 2 + cwc) * (BN / 2) + cl) * 2 + 1];
            float* st = d.stats + (long)(blockIdx.x % d.stats_nrep) * 2 * N;
            atomicAdd(&st[n], s0);
            atomicAdd(&st[N + n], q0);
          }
        }
      }
      constexpr int CPR = BN / OVE;                            // 16-B chunks per tile row
      for (int c = tid; c < BM * CPR; c += 256) {
        const int ml = c / CPR, cc = c % CPR;
        const int m = bm0 + ml, n = bn0 + cc * OVE;
        if (m < M && n < N) *(u32x4*)(C + (long)m * LDC + n) = *(const u32x4*)(sC + ml * SC + cc * 16);
      }
      STAMP(5);
      return;
    }
  }

#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = bn0 + wc * (BN / 2) + j * 16 + lr;
      if (n >= N) continue;
      const float bias = (d.bias && blockIdx.y == 0) ? d.bias[n] : 0.f;
      const int mb = bm0 + wr * (BM / 2) + i * 16 + lg * 4;
      float keep4[4] = {1.f, 1.f, 1.f, 1.f};
      if constexpr (EPI == EPI_HIGHWAY) {
        // one Philox4x32 call serves the lane's 4 consecutive rows
        if (!d.mask && d.use_philox) highway_keep4(d.seed_dev ? *d.seed_dev : d.seed, d.stream, mb >> 2, N, n, d.drop_p, keep4);
      }
      float st_s = 0.f, st_q = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mb + r;
        if (m >= M) continue;
        float v = d.alpha * acc[i][j][r] + bias;
        if constexpr (EPI == EPI_BNSTATS) {
          C[(long)m * LDC + n] = from_f32<TO>(v);
          st_s += v; st_q += v * v;
        } else if constexpr (EPI == EPI_PLAIN || WG) {
          const long o = (long)m * LDC + n;
          if constexpr (sizeof(TO) == 4) {
            if (split) { atomicAdd((float*)&C[o], v); continue; }
          }
          if (d.accumulate) v += to_f32<TO>(C[o]);
          C[o] = from_f32<TO>(v);
        } else {   // EPI_HIGHWAY
          const float y = highway_gate(v, to_f32<TI>(((const TI*)d.X)[(long)m * d.ldx + n]));
          if (d.Hpre) d.Hpre[(long)m * d.ldh + n] = v;          // (null: forward only, nothing saved for a backward pass)
          float keep = keep4[r];
          if (d.mask) keep = (float)d.mask[(long)m * d.ldmask + n];
          if (d.mask_out) d.mask_out[(long)m * d.ldmask_out + n] = (uint8_t)keep;
          C[(long)m * LDC + n] = from_f32<TO>(y * keep * d.keep_scale);
        }
      }
      if constexpr (EPI == EPI_BNSTATS) {
        // column n lives in lanes {lr, lr+16, lr+32, lr+48}: fold the 4 row groups, one atomic pair per column
        st_s += __shfl_xor(st_s, 16, 64); st_q += __shfl_xor(st_q, 16, 64);
        st_s += __shfl_xor(st_s, 32, 64); st_q += __shfl_xor(st_q, 32, 64);
        float* st = d.stats + (long)(blockIdx.x % d.stats_nrep) * 2 * N;
        if (lg == 0) { atomicAdd(&st[n], st_s); atomicAdd(&st[N + n], st_q); }
      }
    }
  }
}
#undef LDC

// ------------------------------------------------------------------------------------------------------------------
// tile8: the bf16 k-contiguous product / implicit-GEMM convolution with EIGHT waves per 128-row tile (2 per SIMD).
//
// Measured on MI355X (tools/gemm_stamps.py) the 4-wave kernel above spends ~1500 cycles per 64-deep K tile where the MFMA
// work is 512: one wave per SIMD serialises its LDS-DMA issue, its fragment reads and its MFMAs, and two tiles in flight do
// not cover the ~2000-cycle loaded DMA latency.  Here a SIMD holds two waves (one can issue DMA / wait on LDS while the
// other feeds the matrix pipe), the ring is NS deep (NS-1 tiles in flight) and addressing is cheap:
//   * tiles reach LDS by `buffer_load_dwordx4 ... lds` behind ONE buffer descriptor per operand: a 32-bit byte offset per
//     chunk, and an offset beyond the descriptor's extent (conv padding, M/N/K tails, tiles past the end of K) reads as
//     zero without touching memory -- no 64-bit address math, no branches, no zero page;
//   * every iteration issues exactly NL DMAs, so the counted s_waitcnt is a constant and the loop body is branch-free.
// Waves are 4 (M) x 2 (N): a wave owns 32 x BN/2 of the tile.  LDS image, swizzle and C/D layout as in the kernel above.
template <typename TO, int BN, int EPI, bool CONV, int NS, bool ABN = false, bool ARES = false, int AMAXK = (ARES ? 2048 : 1024)>
__global__ __launch_bounds__(512) void tile8_kernel(const GemmDesc d, const unsigned a_bytes, const unsigned b_bytes) {
  static_assert(!ARES || ABN, "the residual-on-load form extends the A-side BatchNorm");
  constexpr int BM = 128, BK = 64, NT = 512;
  constexpr int TM = 2, TN = BN / 32;
  constexpr int CA = BM * 8 / NT, CB = BN * 8 / NT;          // 16-B chunks per thread per tile
  constexpr int NL = CA + CB + (ARES ? CA : 0);              // LDS-DMA instructions per thread per stage
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, R_BYTES = ARES ? A_BYTES : 0, STAGE = A_BYTES + B_BYTES + R_BYTES;
  constexpr int OSZ = sizeof(TO), OVE = 16 / OSZ, SC = BN * OSZ + 16;
  constexpr int EPI_BYTES = EPI == EPI_HIGHWAY ? BM * (BN + 4) * 4 : (EPI == EPI_GUMBELMAX ? 8 * BN * 4 : BM * SC + 8 * (BN / 2) * 2 * 4);   // highway stages h in f32
  constexpr int RING_BYTES = NS * STAGE > EPI_BYTES ? NS * STAGE : EPI_BYTES;
  constexpr int ABN_MAXK = AMAXK;                             // A-side BatchNorm: [scale, shift] per input channel behind the ring
  constexpr int SMEM_BYTES = RING_BYTES + (ABN ? ABN_MAXK * 8 : 0) + (ARES ? ABN_MAXK * 8 : 0);     // ARES: + the shortcut's [scale, shift]
  constexpr unsigned OOB = 0x80000000u;                       // >= any extent this kernel is launched with
  static_assert(CB >= 1 && SMEM_BYTES <= 160 * 1024, "tile8 LDS budget");
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  STAMP(0);
  const int wr = w >> 1, wc = w & 1;
  const int lr = lane & 15, lg = lane >> 4;

  const int tiles_m = (d.M + BM - 1) / BM, tiles_n = (d.N + BN - 1) / BN;
  const int bid = xcd_run(blockIdx.x, gridDim.x);
  const int bm0 = (d.n_fast ? bid / tiles_n : bid % tiles_m) * BM;
  const int bn0 = (d.n_fast ? bid % tiles_n : bid / tiles_m) * BN;
  const int M = d.M, N = d.N, K = d.K;

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A, 0, (int)a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)d.B, 0, (int)b_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc((void*)(ARES ? d.res : d.A), 0, (int)a_bytes, 0x00020000);

  // ---- per-thread chunk coordinates: rows (tid>>3) + 64 i, physical chunk slot tid&7 = logical chunk ^ swizzle(row)
  const int kc = swz_dma_chunk(tid) * 8;                       // logical k offset (elements) inside a K tile
  int a_off[CA], a_hi0[CA], a_wi0[CA];
  bool a_ok[CA];
  int cv_r = 0, cv_s = 0, cv_c = 0;
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int m = bm0 + (tid >> 3) + i * 64;
    a_ok[i] = m < M;
    if constexpr (CONV) {
      const ConvOrigin<int> o = conv_origin<int>(m, a_ok[i], d.cHo, d.cWo, d.cH, d.cW, d.cStride, d.cPad);      // (operands under 2 GiB)
      a_hi0[i] = o.hi0; a_wi0[i] = o.wi0;
      a_off[i] = o.pix * d.cCin;
    } else {
      a_hi0[i] = a_wi0[i] = 0;
      a_off[i] = m * (int)d.lda;
    }
  }
  if constexpr (CONV) {
    cv_c = kc % d.cCin;
    const int t = kc / d.cCin;
    cv_s = t % d.cKW;
    cv_r = t / d.cKW;
  }
  int b_off[CB];
  bool b_ok[CB];
#pragma unroll
  for (int i = 0; i < CB; ++i) {
    const int n = bn0 + (tid >> 3) + i * 64;
    b_ok[i] = n < N;
    b_off[i] = n * (int)d.ldb;
  }
  const int wbase = (tid & ~63) * 16;

  // one K tile -> ring stage `st`; called once per kt in increasing order (the conv (r,s,c) runs along)
  auto issue = [&](int kt, int st) {
    unsigned char* sA = smem + st * STAGE;
    unsigned char* sB = sA + A_BYTES;
    const int k = kt * BK + kc;
    const bool kok = k < K;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      unsigned voff;
      if constexpr (CONV) {
        const bool ok = (unsigned)(a_hi0[i] + cv_r) < (unsigned)d.cH & (unsigned)(a_wi0[i] + cv_s) < (unsigned)d.cW & kok;
        voff = ok ? (unsigned)(a_off[i] + (cv_r * d.cW + cv_s) * d.cCin + cv_c) * 2u : OOB;
      } else {
        voff = (a_ok[i] & kok) ? (unsigned)(a_off[i] + k) * 2u : OOB;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_ptr)(sA + i * (NT * 16) + wbase), 16, (int)voff, 0, 0, CONV ? GIC_TRUNK_NT : 0);
      if constexpr (ARES)        // the shortcut tile: same rows and channels of `res`, behind the B tile of the stage
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsR, (lds_void_ptr)(sB + B_BYTES + i * (NT * 16) + wbase), 16, (int)voff, 0, 0, CONV ? GIC_TRUNK_NT : 0);
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      const unsigned voff = (b_ok[i] & kok) ? (unsigned)(b_off[i] + k) * 2u : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_ptr)(sB + i * (NT * 16) + wbase), 16, (int)voff, 0, 0, 0);
    }
    if constexpr (CONV) conv_tap_advance(cv_r, cv_s, cv_c, BK, d.cCin, d.cKW);
  };

  // ---- A-side BatchNorm + ReLU: per-channel [scale, shift] from the producer's sums, then each thread normalises the chunks it
  // DMA'd itself (its own vmcnt wait covers them) in LDS before the barrier publishes the stage.
  float* coef = (float*)(smem + RING_BYTES);
  if constexpr (ABN) {
    const int Cn = CONV ? d.cCin : K;                          // channels of the normalised operand
    for (int c = tid; c < ABN_MAXK; c += NT) {
      float sc = 0.f, sh = 0.f;
      if (c < Cn) {
        float mean, rstd;
        bn_moments(d.in_stats, d.in_nrep, Cn, c, d.in_inv_count, mean, rstd);
        sc = d.in_gamma[c] * rstd;
        sh = d.in_beta[c] - mean * sc;
      }
      coef[2 * c] = sc; coef[2 * c + 1] = sh;
      if constexpr (ARES) {      // the shortcut: its own BatchNorm (projection) or identity (scale 1, shift 0)
        float rs = 1.f, rt = 0.f;
        if (d.res_stats && c < Cn) {
          float mean, rstd;
          bn_moments(d.res_stats, d.res_nrep, Cn, c, d.res_inv_count, mean, rstd);
          rs = d.res_gamma[c] * rstd;
          rt = d.res_beta[c] - mean * rs;
        }
        coef[2 * ABN_MAXK + 2 * c] = rs; coef[2 * ABN_MAXK + 2 * c + 1] = rt;
      }
    }
    __syncthreads();
  }
  const bool wb = ARES && d.out_wb && bn0 == 0;              // first N tile: also materialise the formed operand (the block output)
  auto abn = [&](int kt, int st) {
    if constexpr (ABN) {
      const int k = kt * BK + kc;
      if (k < K) {
        // channel and tap of this thread's chunks (all CA of them share k): a 16-byte chunk never straddles a tap (Cin % 8 == 0)
        const int ch = CONV ? k % d.cCin : k;
        const int tap = CONV ? k / d.cCin : 0;
        const int ts = tap % (CONV ? d.cKW : 1), tr = tap / (CONV ? d.cKW : 1);
        float scl[8], sft[8];
        bn_unpack8(coef + 2 * ch, scl, sft);
        float rsc[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, rsf[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (ARES) bn_unpack8(coef + 2 * ABN_MAXK + 2 * ch, rsc, rsf);
#pragma unroll
        for (int i = 0; i < CA; ++i) {
          // padding taps and rows past M were zero-filled by the DMA and stay zero (the reference pads the NORMALISED tensor)
          const bool ok = CONV ? ((unsigned)(a_hi0[i] + tr) < (unsigned)d.cH & (unsigned)(a_wi0[i] + ts) < (unsigned)d.cW) : a_ok[i];
          if (!ok) continue;
          bf16x8* p = (bf16x8*)(smem + st * STAGE + i * (NT * 16) + tid * 16);
          bf16x8 v = *p;
          if constexpr (ARES) {
            const bf16x8 r = *(const bf16x8*)(smem + st * STAGE + A_BYTES + B_BYTES + i * (NT * 16) + tid * 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (bf16_t)fmaxf((float)v[e] * scl[e] + sft[e] + ((float)r[e] * rsc[e] + rsf[e]), 0.f);
            // 1x1 / stride 1 / pad 0: operand row m, channels k..k+7 = element a_off[i] + k of the [M, Cin] block output
            if (wb) *(bf16x8*)((bf16_t*)d.out_wb + (long)a_off[i] + k) = v;
          } else {
            v = bn_relu8(v, scl, sft);
          }
          *p = v;
        }
      }
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // a whole K tile (the ring-less and 2-stage loops): ALL its fragment reads, then all its MFMAs (read_half / mfma_half below interleave
  // the two halves for the deep ring)
  auto compute = [&](int st) {
    const unsigned char* sA = smem + st * STAGE;
    const unsigned char* sB = sA + A_BYTES;
    bf16x8 fa[2][TM], fb[2][TN];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        const int row = wr * 32 + t * 16 + lr;
        fa[ks][t] = *(const bf16x8*)(sA + row * 128 + swz_chunk(row, ks * 4 + lg));
      }
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const int row = wc * (BN / 2) + t * 16 + lr;
        fb[ks][t] = *(const bf16x8*)(sB + row * 128 + swz_chunk(row, ks * 4 + lg));
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) mfma_block(acc, fa[ks], fb[ks]);
  };

  // fragment reads / MFMAs of one 32-deep half (ks) of a K tile, as separate phases for the software pipeline below
  auto read_half = [&](int st, int ks, bf16x8 (&fa)[TM], bf16x8 (&fb)[TN]) {
    const unsigned char* sA = smem + st * STAGE;
    const unsigned char* sB = sA + A_BYTES;
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      const int row = wr * 32 + t * 16 + lr;
      fa[t] = *(const bf16x8*)(sA + row * 128 + swz_chunk(row, ks * 4 + lg));
    }
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const int row = wc * (BN / 2) + t * 16 + lr;
      fb[t] = *(const bf16x8*)(sB + row * 128 + swz_chunk(row, ks * 4 + lg));
    }
  };
  auto mfma_half = [&](const bf16x8 (&fa)[TM], const bf16x8 (&fb)[TN]) { mfma_block(acc, fa, fb); };

  // ---- K loop: NS-1 tiles in flight.  Tiles past the end of K are all-OOB DMAs (zero fill, no traffic), so the count
  // of outstanding DMAs is the same in every iteration.
  const int nk = (K + BK - 1) / BK;
  STAMP(1);
  if constexpr (NS == 1) {
    // shallow K (one or two tiles): no ring; the LDS footprint is the C tile's, so up to four blocks share a CU and hide
    // each other's load latency and epilogue
    for (int kt = 0; kt < nk; ++kt) {
      if (kt) __builtin_amdgcn_s_barrier();            // every wave is done reading the previous tile
      issue(kt, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      abn(kt, 0);
      __builtin_amdgcn_s_barrier();
      compute(0);
    }
  } else if constexpr (NS < 4) {
    // 2-stage ring: two workgroups share the CU and cover each other's phases; the plain loop measures faster here
    issue(0, 0);
    int st = 0;
    for (int kt = 0; kt < nk; ++kt) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      abn(kt, st);
      __builtin_amdgcn_s_barrier();                      // stage kt published; every wave is done reading stage kt-1
      if (kt == 0) STAMP(2);
      if (!(DBG & 1)) issue(kt + 1, st ^ 1);
      if (!(DBG & 2)) compute(st);
      st ^= 1;
    }
  } else {
    // Software pipeline across K tiles: the second half's fragments of tile kt-1 stay in registers over the barrier, so that
    // every MFMA phase has the next phase's LDS reads in flight under it (all 8 waves leave the barrier in lockstep: without
    // this the CU alternates between an LDS-read phase and an MFMA phase):
    //     barrier | read A(kt) | mfma B(kt-1) | DMA(kt+NS-1) | read B(kt) | mfma A(kt)       A / B = 32-deep halves
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) issue(s, s);
    bf16x8 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
    int st = 0, st_fill = NS - 1;
    for (int kt = 0; kt < nk; ++kt) {
      // stage kt has landed once all but this wave's newest (NS-2) tiles are done.  This wave's reads of stage kt-1 (their
      // data is needed below anyway) must have returned before the barrier lets anyone refill that stage.
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NS >= 2 ? (NS - 2) * NL : 0) : "memory");
      abn(kt, st);
      __builtin_amdgcn_s_barrier();
      if (kt == 0) STAMP(2);
      if (!(DBG & 2)) {
        read_half(st, 0, fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        if (kt > 0) mfma_half(fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (!(DBG & 1)) issue(kt + NS - 1, st_fill);
      if (!(DBG & 2)) {
        __builtin_amdgcn_sched_barrier(0);
        read_half(st, 1, fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_half(fa0, fb0);
      }
      st = st == NS - 1 ? 0 : st + 1;
      st_fill = st_fill == NS - 1 ? 0 : st_fill + 1;
    }
    if (!(DBG & 2) && nk > 0) mfma_half(fa1, fb1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // stray zero-fill DMAs must not land in the C tile
  __syncthreads();
  STAMP(3);

  if constexpr (EPI == EPI_GUMBELMAX) {
    // rows m = vocabulary entries, columns n = roll-out rows.  A lane's four accumulator registers of a 16x16 block are four CONSECUTIVE
    // vocabulary entries of one roll-out row: one Philox4x32 call (or one 16-byte load of explicit uniforms) and one bias load per block.
    float* sV = (float*)smem;                    // [4 (wr)][BN] best value
    int* sI = (int*)(smem + 4 * BN * 4);         // [4 (wr)][BN] its vocabulary index
    const float eps = 1e-10f;                    // generator.py:84
    const uint64_t seed = d.seed_dev ? *d.seed_dev : d.seed;
    const float T = d.gm_temperature;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nl = wc * (BN / 2) + j * 16 + lr;
      const int n = bn0 + nl;
      float best = -INFINITY;
      int best_i = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int m0 = bm0 + wr * 32 + i * 16 + lg * 4;
        if (m0 < M && n < N) {                   // (M % 4 == 0: a quad is inside the vocabulary or past it as a whole)
          const float4 bv = *(const float4*)(d.gm_bias + m0);
          const float bia[4] = {bv.x, bv.y, bv.z, bv.w};
          float uu[4];
          if (d.gm_u) {
            const float4 uv = *(const float4*)(d.gm_u + (long)n * d.gm_ldu + m0);
            uu[0] = uv.x; uu[1] = uv.y; uu[2] = uv.z; uu[3] = uv.w;
          } else {
            uint32_t r0, r1, r2, r3;
            Philox::gen4(seed, d.stream, (uint64_t)n * (uint64_t)(M >> 2) + (uint64_t)(m0 >> 2), r0, r1, r2, r3);
            uu[0] = Philox::u01(r0); uu[1] = Philox::u01(r1); uu[2] = Philox::u01(r2); uu[3] = Philox::u01(r3);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float g = -__logf(-__logf(uu[r] + eps) + eps);      // (bf16 compute mode: the hardware log, as the unfused kernel)
            const float y = (acc[i][j][r] + bia[r] + g) * T;
            if (y > best) { best = y; best_i = m0 + r; }
          }
        }
      }
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {       // the four lane groups hold other vocabulary rows of the same roll-out row
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
      }
      if (lg == 0) { sV[wr * BN + nl] = best; sI[wr * BN + nl] = best_i; }
    }
    __syncthreads();
    if (tid < BN && bn0 + tid < N) {
      float best = sV[tid];
      int best_i = sI[tid];
#pragma unroll
      for (int r = 1; r < 4; ++r) {
        const float ob = sV[r * BN + tid];
        const int oi = sI[r * BN + tid];
        if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
      }
      if (best_i != 0x7fffffff) atomicMax(d.gm_rowkey + bn0 + tid, row_key(best, best_i));
    }
    STAMP(5);
    return;
  }
  TO* __restrict__ C = (TO*)d.C;
  if constexpr (EPI == EPI_HIGHWAY) {
    // h = acc + bias (saved); y = sig(h) relu(h) + (1 - sig(h)) x; C = y * keep * keep_scale.
    // Row-padded bf16 operands only (select_tile8's highway_wide: every leading dimension covers whole 8-column groups, as the
    // discriminator's Fp-padded buffers do; anything else is gemm_kernel's): h goes through LDS and each thread owns a 4-row x 8-column
    // patch = one Philox draw per column (4 rows each), 16-byte accesses to X / Hpre / C and 8-byte ones to the keep mask.  Pad columns
    // of C are written as zero.
    static_assert(sizeof(TO) == 2, "the highway epilogue writes bf16 rows");
    constexpr int SH = BN + 4;
    float* sH = (float*)smem;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nl = wc * (BN / 2) + j * 16 + lr;
      const float bias = (d.bias && bn0 + nl < N) ? d.bias[bn0 + nl] : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) sH[(wr * 32 + i * 16 + lg * 4 + r) * SH + nl] = d.alpha * acc[i][j][r] + bias;
    }
    __syncthreads();
    constexpr int CG = BN / 8;
    const int pc = tid % CG, pr = tid / CG;
    const int n0 = bn0 + pc * 8, m0 = bm0 + pr * 4;
    if (pr < BM / 4 && n0 < N && m0 < M) {
      float keep[8][4];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        keep[e][0] = keep[e][1] = keep[e][2] = keep[e][3] = 1.f;
        if (!d.mask && d.use_philox && n0 + e < N) highway_keep4(d.seed_dev ? *d.seed_dev : d.seed, d.stream, m0 >> 2, N, n0 + e, d.drop_p, keep[e]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + r;
        if (m >= M) break;
        const float4 h0 = *(const float4*)(sH + (pr * 4 + r) * SH + pc * 8), h1 = *(const float4*)(sH + (pr * 4 + r) * SH + pc * 8 + 4);
        const float h[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
        const bf16x8 xv = *(const bf16x8*)((const bf16_t*)d.X + (long)m * d.ldx + n0);
        bf16x8 yv;
        unsigned long long kb = 0ull;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const bool live = n0 + e < N;
          const float y = highway_gate(h[e], (float)xv[e]);
          float k = keep[e][r];
          if (d.mask && live) k = (float)d.mask[(long)m * d.ldmask + n0 + e];
          kb |= (unsigned long long)(live ? (unsigned)k : 0u) << (8 * e);
          yv[e] = (bf16_t)(live ? y * k * d.keep_scale : 0.f);
        }
        if (d.Hpre) {
          *(float4*)(d.Hpre + (long)m * d.ldh + n0) = h0;
          *(float4*)(d.Hpre + (long)m * d.ldh + n0 + 4) = h1;
        }
        if (d.mask_out) *(unsigned long long*)(d.mask_out + (long)m * d.ldmask_out + n0) = kb;
        *(bf16x8*)((bf16_t*)C + (long)m * d.ldc + n0) = yv;
      }
    }
    STAMP(5);
    return;
  }
  // bf16 C += result: straight from the f32 accumulators, rounded ONCE as gemm_kernel does.  (The staged tile below holds the product
  // already rounded to bf16: adding C to that rounds twice and lands up to a whole bf16 ulp from the correctly rounded sum.)  Plain
  // products only: no convolution entry point sets `accumulate` (conv_base declines it), so the staged loop's accumulate branch is
  // live for f32 C alone, where the staged value is unrounded.
  if constexpr (EPI == EPI_PLAIN && !CONV && sizeof(TO) == 2) {
    if (d.accumulate) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = bn0 + wc * (BN / 2) + j * 16 + lr;
        if (n >= N) continue;
        const float bias = d.bias ? d.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = bm0 + wr * 32 + i * 16 + lg * 4 + r;
            if (m >= M) continue;
            const long o = (long)m * d.ldc + n;
            C[o] = from_f32<TO>(d.alpha * acc[i][j][r] + bias + to_f32<TO>(C[o]));
          }
        }
      }
      STAMP(5);
      return;
    }
  }
  // ---- epilogue: C tile through LDS (16-byte row stores), BatchNorm column sums folded across the block
  unsigned char* sC = smem;
  float* sStat = (float*)(smem + BM * SC);                   // [8 waves][BN/2][2]
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wc * (BN / 2) + j * 16 + lr;
    const int n = bn0 + nl;
    const float bias = (d.bias && n < N) ? d.bias[n] : 0.f;
    float st_s = 0.f, st_q = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ml = wr * 32 + i * 16 + lg * 4 + r;
        const float v = d.alpha * acc[i][j][r] + bias;
        *(TO*)(sC + ml * SC + nl * OSZ) = from_f32<TO>(v);
        if (EPI == EPI_BNSTATS && bm0 + ml < M) { st_s += v; st_q += v * v; }
      }
    }
    if constexpr (EPI == EPI_BNSTATS) {
      st_s += __shfl_xor(st_s, 16, 64); st_q += __shfl_xor(st_q, 16, 64);
      st_s += __shfl_xor(st_s, 32, 64); st_q += __shfl_xor(st_q, 32, 64);
      if (lg == 0) { sStat[(w * (BN / 2) + j * 16 + lr) * 2] = st_s; sStat[(w * (BN / 2) + j * 16 + lr) * 2 + 1] = st_q; }
    }
  }
  __syncthreads();
  STAMP(4);
  if constexpr (EPI == EPI_BNSTATS) {
    if (tid < BN) {                                          // column tid: waves (wr = 0..3, wc)
      const int cwc = tid / (BN / 2), cl = tid % (BN / 2), n = bn0 + tid;
      if (n < N) {
        float s0 = 0.f, q0 = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s0 += sStat[((r * 2 + cwc) * (BN / 2) + cl) * 2];
          q0 += sStat[((r * 2 + cwc) * (BN / 2) + cl) * 2 + 1];
        }
        float* stp = d.stats + (long)(blockIdx.x % d.stats_nrep) * 2 * N;
        atomicAdd(&stp[n], s0);
        atomicAdd(&stp[N + n], q0);
      }
    }
  }
  // (its own row-store loop: the f32 accumulate branch exists here only)
  constexpr int CPR = BN / OVE;                              // 16-B chunks per tile row
  for (int c = tid; c < BM * CPR; c += NT) {
    const int ml = c / CPR, cc = c % CPR;
    const int m = bm0 + ml, n = bn0 + cc * OVE;
    if (m < M && n < N) {
      u32x4 v = *(const u32x4*)(sC + ml * SC + cc * 16);
      if (d.accumulate) {                                    // f32 C += result (gradients accumulated across passes); bf16: see above
        const u32x4 o = *(const u32x4*)(C + (long)m * d.ldc + n);
        TO* pv = (TO*)&v;
        const TO* po = (const TO*)&o;
#pragma unroll
        for (int e = 0; e < OVE; ++e) pv[e] = from_f32<TO>(to_f32<TO>(pv[e]) + to_f32<TO>(po[e]));
      }
      *(u32x4*)(C + (long)m * d.ldc + n) = v;
    }
  }
  STAMP(5);
}

// ---------------------------------------------------------------------------------------------------- selection (pure host code)

// tile8_kernel<TO, BN, EPI, CONV, NS, ABN, ARES, AMAXK>; TO, EPI and CONV are the descriptor's
struct Tile8Plan { int BN, NS; bool abn, ares; int amaxk; unsigned grid, a_bytes, b_bytes; };
// gemm_kernel<TI, TO, AKC, BKC, BM, BM, VEC, EPI, CONV, PIPE> over dim3(tiles, splits), `per` K tiles per split; zero_grid > 0: C is
// zero-filled first (split-K adds into it)
struct Gemm4Plan { int bm; bool vec, pipe; int tiles, splits, per, zero_grid; bool wg; };      // wg: the EPI_WGRAD form (gemm.h's weight-gradient extras)

enum Family { F_NONE = 0, F_STEM, F_PATCH, F_STREAM, F_PIX, F_PANEL, F_TILE8, F_GEMM4 };

struct Plan {
  int family = F_NONE;
  GemmDesc d;               // what the 8-wave and 4-wave kernels take as their argument (tile8: with n_fast chosen)
  StemPlan stem; PatchPlan patch; StreamPlan strm; PixPlan pix; PanelPlan panel; Tile8Plan t8; Gemm4Plan g4;
};

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

// Elements spanned by a k-contiguous [rows, K] operand with leading dimension ld: what a buffer descriptor over it must cover
long kc_extent(int rows, long ld, int K) { return (long)(rows - 1) * ld + K; }
bool under_2g(long bf16_elems) { return bf16_elems * 2 < (1l << 31); }

// What tile8's highway epilogue presumes (its 4-row x 8-column patches): bf16 C, every leading dimension covering whole 8-column groups
// and divisible as its 16- / 8-byte accesses need, 16-byte aligned C / X / Hpre, an 8-byte aligned mask_out.  The discriminator's
// Fp-padded buffers; any other highway product is gemm_kernel's.
bool highway_wide(const GemmDesc& d) {
  const int n8 = (d.N + 7) & ~7;
  return d.out_dtype == DT_BF16 && d.ldc >= n8 && d.ldx >= n8 && d.ldh >= n8 && (!d.mask_out || d.ldmask_out >= n8) &&
         d.ldc % 8 == 0 && d.ldx % 8 == 0 && d.ldh % 4 == 0 && (!d.mask_out || d.ldmask_out % 8 == 0) &&
         aligned16(d.C) && aligned16(d.X) && aligned16(d.Hpre) && (((uintptr_t)d.mask_out) & 7) == 0;
}

// The 8-wave kernel qualifies: bf16 k-contiguous operands under 2 GiB each, a plain (overwrite or accumulate, f32 or bf16 C) / BatchNorm-sum
// epilogue onto a 16-byte-aligned C whose N and ldc are whole 16-byte chunks (or the row-padded highway epilogue).  false: fall back to
// gemm_kernel.
bool select_tile8(const GemmDesc& d, Tile8Plan& p, int& n_fast) {
  static const bool off = getenv("GIC_NO_TILE8") != nullptr;
  static const int big_min = env_int("GIC_TILE8_BIG_MIN", 160), ns2_tiles = env_int("GIC_TILE8_NS2_TILES", 256), min_nk = env_int("GIC_TILE8_MIN_NK", 1);
  static const int res_ns = env_int("GIC_TILE8_RES_NS", 1), ns1_nk = env_int("GIC_TILE8_NS1_NK", 4);
  const int OVE = 16 / dtype_size(d.out_dtype);
  const bool highway = d.epi == EPI_HIGHWAY;
  if (off || d.M < 128) return false;
  if (!highway && ((d.N % OVE) || (d.ldc % OVE) || !aligned16(d.C))) return false;
  if (highway && (d.in_dtype != DT_BF16 || !highway_wide(d))) return false;
  const long small_tiles = (long)cdiv(d.M, 128) * cdiv(d.N, 64), big_tiles = (long)cdiv(d.M, 128) * cdiv(d.N, 128);
  // a plain product must fill the chip with 128-row tiles and be deep enough to amortise the ring (else: gemm_kernel, split-K)
  if (!d.conv && (small_tiles < 128 || d.K < 256)) return false;
  const long a_elems = d.conv ? (long)(d.M / (d.cHo * d.cWo)) * d.cH * d.cW * d.cCin : kc_extent(d.M, d.lda, d.K);
  const long b_elems = kc_extent(d.N, d.ldb, d.K);
  if (!under_2g(a_elems) || !under_2g(b_elems)) return false;
  const int nk = cdiv(d.K, 64);
  if (nk < min_nk) return false;
  p.a_bytes = (unsigned)(a_elems * 2); p.b_bytes = (unsigned)(b_elems * 2);
  p.abn = p.ares = false; p.amaxk = 1024;
  // deep ring (4 stages, 128 KB: one block per CU) when the grid is about one block per CU; with several blocks per CU a
  // 2-stage ring (64 KB) lets two blocks share the CU so one block's epilogue runs under the other's K loop
  bool n128;
  if (d.epi == EPI_BNSTATS && d.conv && d.in_stats && d.res) {
    // + residual on load: 1x1 / stride 1 / pad 0 only, one- or two-stage ring (two tiles per stage on the A side)
    if (d.cKH != 1 || d.cKW != 1 || d.cStride != 1 || d.cPad != 0 || d.cCin % 8 || d.cCin > 2048 || !bn_in_args_ok(d) ||
        (d.res_stats && (!d.res_gamma || !d.res_beta || d.res_inv_count <= 0.f)))
      return false;
    // ring-less (one stage: two A-side tiles + B): 2-3 workgroups share a CU and cover each other's DMA latency and LDS rewrite;
    // the coefficient table is sized by the channel count (512 -> 8 KB, 2048 -> 32 KB)
    n128 = d.N >= 128;
    p.abn = p.ares = true; p.amaxk = d.cCin <= 512 ? 512 : 2048;
    p.NS = res_ns == 1 ? 1 : 2;
  } else if (d.epi == EPI_BNSTATS && d.conv && d.in_stats) {
    // A-side BatchNorm + ReLU: whole 16-byte chunks per tap, channels within the LDS table
    if (d.cCin % 8 || d.cCin > 1024 || !bn_in_args_ok(d)) return false;
    n128 = d.N >= 128 && big_tiles >= big_min;
    const long tiles = n128 ? big_tiles : small_tiles;
    p.abn = true;
    p.NS = nk <= 4 && tiles > 512 ? 1 : (tiles > 256 ? 2 : 4);
  } else if (!highway && nk <= ns1_nk && (d.N >= 128 ? big_tiles : small_tiles) > 512) {
    n128 = d.N >= 128;
    p.NS = 1;
  } else {
    n128 = d.N >= 128 && big_tiles >= big_min;
    p.NS = (n128 ? big_tiles : small_tiles) > ns2_tiles ? 2 : 4;
  }
  p.BN = n128 ? 128 : 64;
  p.grid = (unsigned)(n128 ? big_tiles : small_tiles);
  // what an XCD's concurrent workgroups share (common.h): A bytes actually gathered (a strided 1x1 touches 1 / stride^2 of its input)
  n_fast = xcd_share_a(2 * (a_elems < (long)d.M * d.K ? a_elems : (long)d.M * d.K), 2l * d.N * d.K, cdiv(d.N, d.N >= 128 ? 128 : 64));
  return true;
}

// What the weight-gradient extras (a_sum / a_sum2, C2 / n_split) need of a product, the chosen tile apart: gemm_kernel's vectorised
// m/n-contiguous plain form in bf16 compute mode, outside the deterministic mode (its sums are per-split atomics), over a C that the
// launch itself zero-fills, and only for a descriptor that says `wgrad` (the extras' fields are union members, gemm.h).  The f32 parity
// mode is left out: it is not required, and with an f32 form of this fold in the tree the eager-against-graph comparison of the f32 train
// step (tests/test_gpu_step.py) failed in 3 of 6 runs where it passes without; the cause of that was not established.
bool wgrad_form(const GemmDesc& d, bool vec) {
  return d.wgrad && !d.conv && !d.a_kc && !d.b_kc && d.epi == EPI_PLAIN && d.in_dtype == DT_BF16 && vec && !d.c_zeroed && !det_mode();
}
// gemm()'s `vec` of a plain product: what the predicates below and gemm() itself both go by
bool plain_vec(const GemmDesc& d) {
  const int ve = 16 / dtype_size(d.in_dtype);
  bool vec = aligned16(d.A) && aligned16(d.B) && (d.lda % ve == 0) && (d.ldb % ve == 0);
  if (d.a_kc || d.b_kc) vec = vec && (d.K % ve == 0);
  return vec;
}

// The 4-wave kernel takes every product the validation lets through: tile size, split-K and the pipeline
void select_gemm4(const GemmDesc& d, bool vec, Gemm4Plan& p) {
  // 128x128 tiles only when there are enough of them to co-schedule two blocks per CU (latency hiding by TLP), else 64x64;
  // GIC_GEMM_BIG_MIN overrides the threshold for tuning runs
  static const int big_min = env_int("GIC_GEMM_BIG_MIN", 192);
  const long big_tiles = (long)cdiv(d.M, 128) * cdiv(d.N, 128);
  p.bm = big_tiles >= big_min && d.N >= 128 && (d.conv || d.M >= 128) ? 128 : 64;
  p.vec = vec;
  const bool bf16_in = d.in_dtype == DT_BF16;
  p.tiles = cdiv(d.M, p.bm) * cdiv(d.N, p.bm);
  const int tiles = p.tiles, nk = cdiv(d.K, bf16_in ? 64 : 32);
  // split-K only where the tile grid leaves most of the 256 CUs idle and K is deep enough to share
  int splits = 1;
  // (bf16 compute mode only: the f32 parity mode stays bit-reproducible run to run, atomics reorder the f32 sum)
  if (d.epi == EPI_PLAIN && bf16_in && d.out_dtype == DT_F32 && !d.no_split) {
    if (tiles < 24 && nk >= 8) {                 // skinny recurrent / head products: fill the chip
      splits = 256 / tiles;
      if (splits > nk / 2) splits = nk / 2;
      if (splits > 16) splits = 16;
    } else if (tiles <= 192 && nk >= 32) {       // deep-K gradients over few tiles (K = B*L or V): ~2 blocks per CU
      splits = 512 / tiles;
      if (splits > nk / 8) splits = nk / 8;
      if (splits > 16) splits = 16;
    } else if (!d.a_kc && !d.b_kc && tiles <= 192 && nk >= 16) {   // weight-gradient form (both operands row-major over K = B*L rows) over few tiles:
      splits = 512 / tiles;                      // the D embedding gradient, 157 tiles x K = 1280
      if (splits > nk / 4) splits = nk / 4;
    } else if (tiles <= 320 && nk >= 64) {       // about one 4-wave block per CU over a very deep K (the highway weight gradient: 225 tiles,
      splits = 768 / tiles;                      // K = 2B*R = 8192): ~3 blocks per CU, 87 -> 47 us (tools/gemm_hw_bench.py)
    }
    if (splits < 1) splits = 1;
    // deterministic mode: two splits add onto a zeroed C in either order to the same bits, ((0 + a) + b == (0 + b) + a); more
    // splits, or two onto a C being accumulated into, do not
    if (det_mode()) splits = (d.accumulate || splits < 2) ? 1 : 2;
  }
  // K = 0 (the empty sum, C = bias (+ C)): one split of no K tiles, the kernel's K loop does not run and its epilogue writes C
  p.per = nk ? cdiv(nk, splits) : 1;
  p.splits = nk ? cdiv(nk, p.per) : 1;
  p.zero_grid = 0;
  if (p.splits > 1 && !d.accumulate && !d.c_zeroed) {
    const long total = (long)d.M * d.N;
    p.zero_grid = (int)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
  }
  // LDS-DMA ring (PIPE) vs register staging: the ring hides load latency when a CU holds ONE block (grid <= ~2 blocks
  // per CU) and K is deep; with many blocks per CU the register-staged kernel wins (2 co-resident blocks, 72 KB LDS each)
  // and for K of one or two tiles the ring's prologue is pure overhead.  Measured on MI355X (tools/gemm_bench.py).
  static const bool no_pipe = getenv("GIC_GEMM_NO_PIPE") != nullptr;
  p.pipe = d.a_kc && d.b_kc && vec && p.per >= 6 && (long)tiles * p.splits <= 2 * 256 + 8 && !no_pipe;
  p.wg = wgrad_form(d, vec) && (d.a_sum || d.C2);      // (in that form alone the unions of gemm.h hold these)
}

// The one list of candidates, in the order they are tried; `after`: the families up to and including it are skipped (the launch of that one
// was refused its LDS grant).  GIC_OK with p.family set, or the status gemm() answers.
int select(const GemmDesc& d, bool vec, int after, Plan& p) {
  const bool bf16_in = d.in_dtype == DT_BF16, bf16_out = d.out_dtype == DT_BF16;
  if (!((d.in_dtype == DT_F32 && d.out_dtype == DT_F32) || (bf16_in && (d.out_dtype == DT_F32 || bf16_out)))) {
    set_last_error("gemm: unsupported dtypes in=%d out=%d", d.in_dtype, d.out_dtype);
    return GIC_ERR_UNSUPPORTED;
  }
  if (d.conv) {
    if (!vec || !d.a_kc || !d.b_kc) { set_last_error("gemm: convolution needs 16-B aligned NHWC / KRSC operands"); return GIC_ERR_UNSUPPORTED; }
    if (bf16_in != bf16_out || (d.epi != EPI_BNSTATS && d.epi != EPI_PLAIN)) {
      set_last_error("gemm: unsupported convolution epilogue / dtype");
      return GIC_ERR_UNSUPPORTED;
    }
  } else if (d.epi != EPI_PLAIN && d.epi != EPI_HIGHWAY) {
    set_last_error("gemm: unknown epilogue %d", d.epi);
    return GIC_ERR_UNSUPPORTED;
  }
  auto take = [&](int family) { p.family = family; return GIC_OK; };
  if (d.conv && bf16_out && d.epi == EPI_BNSTATS) {
    // the stem (7 x 8 window over the zero-bordered NHWC4 image): input rows rolling through an LDS ring (conv_stem.hip)
    if (after < F_STEM && select_conv_stem(d, p.stem)) return take(F_STEM);
    // 3x3 / stride 1: the input patch stays in LDS for all nine taps (conv3x3.hip).  BatchNorm on load of any other window than
    // 1x1 exists there only (tile8 would re-normalise the tile once per tap: slower than the separate pass it replaces).
    if (after < F_PATCH && select_conv3x3_patch(d, p.patch)) return take(F_PATCH);
    // shallow 1x1 layers over many rows: persistent workgroups, resident weights, A tiles streamed across row tiles (conv1x1_stream.hip)
    if (after < F_STREAM && select_conv1x1_stream(d, p.strm)) return take(F_STREAM);
    if (d.stats_only) return GIC_ERR_UNSUPPORTED;               // the statistics-only pass exists there only (no message: callers probe)
    // K = 256 | 512 of a normalised input into many output channels: the pixels in registers, weight tiles streamed (conv1x1_pix.hip)
    if (after < F_PIX && select_conv1x1_pix(d, p.pix)) return take(F_PIX);
    // K = 256 into many output channels: the A panel of a row tile loaded / normalised once for all its channel tiles (conv1x1_panel.hip)
    if (after < F_PANEL && select_conv1x1_panel(d, p.panel)) return take(F_PANEL);
    if (d.in_stats && d.cKH * d.cKW > 1) return GIC_ERR_UNSUPPORTED;
  }
  // the 8-wave kernel: every other bf16 convolution and the wide, deep plain / highway products with k-contiguous operands
  if (after < F_TILE8 && bf16_in && (d.conv || (d.a_kc && d.b_kc && vec))) {
    p.d = d;
    if (select_tile8(d, p.t8, p.d.n_fast)) return take(F_TILE8);
  }
  if (d.conv && d.in_stats) return GIC_ERR_UNSUPPORTED;         // the A-side BatchNorm exists in tile8 only (no message: callers probe)
  // the 4-wave kernel: any layout of a plain product, k-contiguous operands otherwise
  if (!(d.a_kc && d.b_kc) && (d.epi != EPI_PLAIN || d.b_kc)) {
    set_last_error("gemm: unsupported layout a_kc=%d b_kc=%d epi=%d", d.a_kc, d.b_kc, d.epi);
    return GIC_ERR_UNSUPPORTED;
  }
  p.d = d;
  select_gemm4(d, vec, p.g4);
  if (!d.conv && d.epi == EPI_PLAIN && d.C2 && !(p.g4.wg && d.n_split > 0 && d.n_split < d.N && d.n_split % p.g4.bm == 0)) {
    // (a_sum alone is optional: a kernel that cannot fold it runs the product as ever, callers ask wgrad_folds_a_sum first)
    set_last_error("gemm: a second output needs the vectorised weight-gradient form and n_split (%d) on a tile boundary (%d)", d.n_split, p.g4.bm);
    return GIC_ERR_UNSUPPORTED;
  }
  return take(F_GEMM4);
}

// The smallest column count N (roll-out rows) from which gemm_gumbelmax takes an M x N x K product of bf16 k-contiguous operands with
// these leading dimensions (16-byte aligned pointers, a positive temperature and operands under 2 GiB presumed): at least 128 columns and
// 160 tiles of 128 x 128.  0: never (f32, M below 128 or no multiple of 4, the GIC_NO_TILE8 / GIC_NO_FUSED_GUMBELMAX switches).
long gumbelmax_from_cols(int in_dtype, int M, int K, long lda, long ldb) {
  static const bool off = getenv("GIC_NO_TILE8") != nullptr || getenv("GIC_NO_FUSED_GUMBELMAX") != nullptr;
  if (off || in_dtype != DT_BF16 || M < 128 || M % 4 || K % 8 || lda % 8 || ldb % 8 || !under_2g(kc_extent(M, lda, K))) return 0;
  const long mt = cdiv(M, 128), nt = (160 + mt - 1) / mt;           // column tiles that make 160 tiles
  return 128 * (nt - 1) + 1 > 128 ? 128 * (nt - 1) + 1 : 128;
}

// gemm_gumbelmax's one candidate: the 8-wave kernel with 128 x 128 tiles
bool select_gumbelmax(const GemmDesc& d0, Plan& p) {
  GemmDesc& d = p.d = d0;
  const long from = gumbelmax_from_cols(d.in_dtype, d.M, d.K, d.lda, d.ldb);
  if (!from || d.N < from || !d.a_kc || !d.b_kc || !aligned16(d.A) || !aligned16(d.B) || !aligned16(d.gm_bias) ||
      (d.gm_u && (!aligned16(d.gm_u) || d.gm_ldu % 4)) || !(d.gm_temperature > 0.f))
    return false;
  const long a_elems = kc_extent(d.M, d.lda, d.K), b_elems = kc_extent(d.N, d.ldb, d.K);
  const long tiles = (long)cdiv(d.M, 128) * cdiv(d.N, 128);
  if (!under_2g(b_elems)) return false;
  d.epi = EPI_GUMBELMAX;
  d.n_fast = xcd_share_a(2l * d.M * d.K, 2l * d.N * d.K, cdiv(d.N, 128));
  p.t8 = {128, tiles > 256 ? 2 : 4, false, false, 1024, (unsigned)tiles, (unsigned)(a_elems * 2), (unsigned)(b_elems * 2)};
  p.family = F_TILE8;
  return true;
}

// ---------------------------------------------------------------------------------------------------- launch (no shape logic)

__global__ void zero2d_kernel(float* __restrict__ C, long ldc, int M, int N) {
  const long total = (long)M * N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
    C[(i / N) * ldc + (i % N)] = 0.f;
}

// split-K over the weight-gradient extras: both output matrices and the column sums start from zero
__global__ void zero_wgrad_kernel(float* __restrict__ C, long ldc, float* __restrict__ C2, long ldc2, int n_split, float* __restrict__ s1,
                                  float* __restrict__ s2, int M, int N) {
  const long total = (long)M * N, i0 = (long)blockIdx.x * blockDim.x + threadIdx.x, step = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < total; i += step) {
    const long m = i / N;
    const int n = (int)(i - m * N);
    if (C2 && n >= n_split) C2[m * ldc2 + (n - n_split)] = 0.f;
    else C[m * ldc + n] = 0.f;
  }
  for (long m = i0; m < M; m += step) {
    if (s1) s1[m] = 0.f;
    if (s2) s2[m] = 0.f;
  }
}

template <typename TO, int EPI, bool CONV, int BN, int NS, bool ABN = false, bool ARES = false, int AMAXK = 1024>
void launch_tile8_as(const Plan& p, hipStream_t stream) {
  // BatchNorm on load exists under the convolutions' BatchNorm-sum epilogue only; the ring-less form is never selected under the highway
  // epilogue (a plain `if`: that instantiation stays in the code object, without a host stub)
  if constexpr (!ABN || (EPI == EPI_BNSTATS && CONV))
    if (EPI != EPI_HIGHWAY || NS != 1)
      hipLaunchKernelGGL((tile8_kernel<TO, BN, EPI, CONV, NS, ABN, ARES, AMAXK>), dim3(p.t8.grid), dim3(512), 0, stream, p.d, p.t8.a_bytes, p.t8.b_bytes);
}

constexpr int t8_key(int BN, int NS, bool abn = false, bool ares = false, int amaxk = 1024) { return BN + NS * 256 + abn * 2048 + ares * 4096 + amaxk * 8192; }

template <typename TO, int EPI, bool CONV>
void launch_tile8_variant(const Plan& p, hipStream_t stream) {
  const Tile8Plan& t = p.t8;
  switch (t8_key(t.BN, t.NS, t.abn, t.ares, t.amaxk)) {
#define GIC_T8(...) case t8_key(__VA_ARGS__): return launch_tile8_as<TO, EPI, CONV, __VA_ARGS__>(p, stream)
    GIC_T8(128, 1); GIC_T8(128, 2); GIC_T8(128, 4); GIC_T8(64, 1); GIC_T8(64, 2); GIC_T8(64, 4);
    GIC_T8(128, 1, true); GIC_T8(128, 2, true); GIC_T8(128, 4, true); GIC_T8(64, 1, true); GIC_T8(64, 2, true); GIC_T8(64, 4, true);
    GIC_T8(128, 1, true, true, 512); GIC_T8(128, 2, true, true, 512); GIC_T8(64, 1, true, true, 512); GIC_T8(64, 2, true, true, 512);
    GIC_T8(128, 1, true, true, 2048); GIC_T8(128, 2, true, true, 2048); GIC_T8(64, 1, true, true, 2048); GIC_T8(64, 2, true, true, 2048);
#undef GIC_T8
  }
}

void launch_tile8(const Plan& p, hipStream_t stream) {
  const GemmDesc& d = p.d;
  const bool bf16_out = d.out_dtype == DT_BF16;
  if (d.epi == EPI_GUMBELMAX) {
    if (p.t8.NS == 2) launch_tile8_as<float, EPI_GUMBELMAX, false, 128, 2>(p, stream);
    else launch_tile8_as<float, EPI_GUMBELMAX, false, 128, 4>(p, stream);
  } else if (d.conv) {
    if (d.epi == EPI_BNSTATS) launch_tile8_variant<bf16_t, EPI_BNSTATS, true>(p, stream);
    else launch_tile8_variant<bf16_t, EPI_PLAIN, true>(p, stream);
  } else if (d.epi == EPI_HIGHWAY) {
    launch_tile8_variant<bf16_t, EPI_HIGHWAY, false>(p, stream);        // (select_tile8's highway_wide: bf16 C)
  } else {
    if (bf16_out) launch_tile8_variant<bf16_t, EPI_PLAIN, false>(p, stream);
    else launch_tile8_variant<float, EPI_PLAIN, false>(p, stream);
  }
}

template <typename TI, typename TO, bool AKC, bool BKC, int BM, bool VEC, int EPI, bool CONV>
void launch_gemm4_as(const Plan& p, hipStream_t stream) {
  const dim3 grid(p.g4.tiles, p.g4.splits);
  if constexpr (AKC && BKC && VEC) {
    if (p.g4.pipe) {
      hipLaunchKernelGGL((gemm_kernel<TI, TO, AKC, BKC, BM, BM, VEC, EPI, CONV, true>), grid, dim3(256), 0, stream, p.d, p.g4.per);
      return;
    }
  }
  hipLaunchKernelGGL((gemm_kernel<TI, TO, AKC, BKC, BM, BM, VEC, EPI, CONV, false>), grid, dim3(256), 0, stream, p.d, p.g4.per);
}

template <typename TI, typename TO, bool AKC, bool BKC, int EPI, bool CONV>
void launch_gemm4_tile(const Plan& p, hipStream_t stream) {
  const bool big = p.g4.bm == 128;
  if (CONV || p.g4.vec) return big ? launch_gemm4_as<TI, TO, AKC, BKC, 128, true, EPI, CONV>(p, stream) : launch_gemm4_as<TI, TO, AKC, BKC, 64, true, EPI, CONV>(p, stream);
  if constexpr (!CONV && EPI != EPI_WGRAD) return big ? launch_gemm4_as<TI, TO, AKC, BKC, 128, false, EPI, CONV>(p, stream) : launch_gemm4_as<TI, TO, AKC, BKC, 64, false, EPI, CONV>(p, stream);
}

template <typename TI, typename TO>
void launch_gemm4_typed(const Plan& p, hipStream_t stream) {
  const GemmDesc& d = p.d;
  if (d.conv) {
    if constexpr (sizeof(TI) == sizeof(TO)) {
      if (d.epi == EPI_BNSTATS) launch_gemm4_tile<TI, TO, true, true, EPI_BNSTATS, true>(p, stream);
      else launch_gemm4_tile<TI, TO, true, true, EPI_PLAIN, true>(p, stream);
    }
  } else if (d.epi == EPI_HIGHWAY) {
    launch_gemm4_tile<TI, TO, true, true, EPI_HIGHWAY, false>(p, stream);
  } else if (d.a_kc) {
    if (d.b_kc) launch_gemm4_tile<TI, TO, true, true, EPI_PLAIN, false>(p, stream);
    else launch_gemm4_tile<TI, TO, true, false, EPI_PLAIN, false>(p, stream);
  } else if (p.g4.wg) {
    if constexpr (sizeof(TI) == 2) launch_gemm4_tile<TI, TO, false, false, EPI_WGRAD, false>(p, stream);       // (wgrad_form: bf16, vectorised)
  } else {
    launch_gemm4_tile<TI, TO, false, false, EPI_PLAIN, false>(p, stream);
  }
}

void launch_gemm4(const Plan& p, hipStream_t stream) {
  const GemmDesc& d = p.d;
  if (p.g4.wg) {
    g_wgrad_launches.fetch_add(1, std::memory_order_relaxed);
    if (d.C2) g_wgrad_two.fetch_add(1, std::memory_order_relaxed);
  }
  if (p.g4.zero_grid && p.g4.wg)
    hipLaunchKernelGGL(zero_wgrad_kernel, dim3(p.g4.zero_grid), dim3(256), 0, stream, (float*)d.C, d.ldc, (float*)d.C2, d.ldc2, d.n_split, d.a_sum, d.a_sum2, d.M, d.N);
  else if (p.g4.zero_grid) hipLaunchKernelGGL(zero2d_kernel, dim3(p.g4.zero_grid), dim3(256), 0, stream, (float*)d.C, d.ldc, d.M, d.N);
  if (d.in_dtype == DT_F32) launch_gemm4_typed<float, float>(p, stream);
  else if (d.out_dtype == DT_F32) launch_gemm4_typed<bf16_t, float>(p, stream);
  else launch_gemm4_typed<bf16_t, bf16_t>(p, stream);
}

// false: the kernel's LDS grant was refused (the caller selects again, past this family)
bool launch(const Plan& p, hipStream_t stream) {
  switch (p.family) {
    case F_STEM: return launch_conv_stem(p.stem, stream);
    case F_PATCH: return launch_conv3x3_patch(p.patch, stream);
    case F_STREAM: return launch_conv1x1_stream(p.strm, stream);
    case F_PIX: return launch_conv1x1_pix(p.pix, stream);
    case F_PANEL: return launch_conv1x1_panel(p.panel, stream);
    case F_TILE8: launch_tile8(p, stream); return true;
    default: launch_gemm4(p, stream); return true;
  }
}

const char* const kFamily[] = {"none", "conv stem", "conv3x3 patch", "conv1x1 stream", "conv1x1 pix", "conv1x1 panel", "gemm tile8", "gemm"};

// The plan as one line: the kernel with its template arguments in their order, grid, block, dynamic LDS bytes and, for the 4-wave kernel,
// the split of K
void write_route(const Plan& p) {
  char* s = route_line();
  const GemmDesc& d = p.d;
  const char* tn[] = {"f32", "bf16"};
  auto b = [](bool v) { return v ? "true" : "false"; };
  switch (p.family) {
    case F_STEM: snprintf(s, kRouteLen, "conv_stem grid=%u block=512 lds=%zu", p.stem.grid, p.stem.lds); break;
    case F_PATCH: snprintf(s, kRouteLen, "conv3x3_patch<%d,%d,%s,%s> grid=%u block=512 lds=%zu", p.patch.BN, p.patch.P, b(p.patch.multi), b(p.patch.abn), p.patch.grid, p.patch.lds); break;
    case F_STREAM: snprintf(s, kRouteLen, "conv1x1_stream<%d,%d,%s,%s> grid=%u block=512 lds=%zu", p.strm.BN, p.strm.KT, b(p.strm.abn), b(p.strm.stats), p.strm.grid, p.strm.lds); break;
    case F_PIX: snprintf(s, kRouteLen, "conv1x1_pix<%d,%d,%s> grid=%u block=512 lds=%zu", p.pix.K, p.pix.NSTG, b(p.pix.turn), p.pix.grid, p.pix.lds); break;
    case F_PANEL: snprintf(s, kRouteLen, "conv1x1_panel<%d,%s> grid=%u block=512 lds=%zu", p.panel.KT, b(p.panel.abn), p.panel.grid, p.panel.lds); break;
    case F_TILE8:
      snprintf(s, kRouteLen, "tile8<%s,%d,%d,%s,%d,%s,%s,%d> grid=%u block=512 lds=0", d.epi == EPI_GUMBELMAX ? "f32" : tn[d.out_dtype], p.t8.BN, d.epi, b(d.conv),
               p.t8.NS, b(p.t8.abn), b(p.t8.ares), p.t8.amaxk, p.t8.grid);
      break;
    default:
      snprintf(s, kRouteLen, "gemm<%s,%s,%s,%s,%d,%d,%s,%d,%s,%s> grid=%dx%d block=256 lds=0 splits=%d per=%d pipe=%d zero=%d", tn[d.in_dtype], tn[d.out_dtype],
               b(d.a_kc), b(d.b_kc), p.g4.bm, p.g4.bm, b(d.conv || p.g4.vec), d.epi, b(d.conv), b(p.g4.pipe), p.g4.tiles, p.g4.splits, p.g4.splits, p.g4.per,
               (int)p.g4.pipe, p.g4.zero_grid);
      if (p.g4.wg) {      // (a descriptor without the weight-gradient extras keeps its line)
        const size_t n = strlen(s);
        snprintf(s + n, kRouteLen - n, " a_sum=%d n_split=%d", d.a_sum ? (d.a_sum2 ? 2 : 1) : 0, d.C2 ? d.n_split : 0);
      }
  }
}

}  // namespace

bool conv_base(const GemmDesc& d, long a_elems, long b_elems, ConvBase& b) {
  if (!d.conv || d.epi != EPI_BNSTATS || !d.stats || d.in_dtype != DT_BF16 || d.out_dtype != DT_BF16) return false;
  if (d.bias || d.alpha != 1.f || d.accumulate || !aligned16(d.A) || !aligned16(d.B) || !aligned16(d.C)) return false;
  if (d.in_stats && (!bn_in_args_ok(d) || d.in_nrep < 1)) return false;
  if (a_elems * 2 >= (1l << 31) || b_elems * 2 >= (1l << 31)) return false;
  b.A = d.A; b.B = d.B; b.C = d.C; b.stats = d.stats;
  b.in_stats = d.in_stats; b.in_gamma = d.in_gamma; b.in_beta = d.in_beta;
  b.M = d.M; b.N = d.N; b.lda = (int)d.lda; b.ldb = (int)d.ldb; b.ldc = (int)d.ldc;
  b.stats_nrep = d.stats_nrep < 1 ? 1 : d.stats_nrep; b.in_nrep = d.in_nrep; b.in_inv_count = d.in_inv_count;
  b.a_bytes = (unsigned)(a_elems * 2); b.b_bytes = (unsigned)(b_elems * 2);
  return true;
}

void wgrad_launch_counts(long* launches, long* two_matrix) {
  if (launches) *launches = g_wgrad_launches.load(std::memory_order_relaxed);
  if (two_matrix) *two_matrix = g_wgrad_two.load(std::memory_order_relaxed);
}

bool wgrad_folds_a_sum(const GemmDesc& d) { return d.a_sum && wgrad_form(d, plain_vec(d)); }

int wgrad_tile_n(const GemmDesc& d) {
  const bool vec = plain_vec(d);
  if (!wgrad_form(d, vec)) return 0;
  Gemm4Plan p;
  select_gemm4(d, vec, p);
  return p.bm;
}

long gemm_gumbelmax_from_cols(int in_dtype, int M, int K, long lda, long ldb) { return gumbelmax_from_cols(in_dtype, M, K, lda, ldb); }

int gemm_gumbelmax(const GemmDesc& d, hipStream_t stream) {
  GIC_CHECK_ARG(d.A && d.B && d.gm_rowkey && d.gm_bias, "gemm_gumbelmax: null operand");
  Plan p;
  const bool ok = select_gumbelmax(d, p), probe = route_only();
  if (probe && ok) write_route(p);
  if (probe && !ok) snprintf(route_line(), kRouteLen, "unsupported");
  if (!ok) return GIC_ERR_UNSUPPORTED;                     // (no message: callers probe)
  if (probe) return GIC_OK;
  launch_tile8(p, stream);
  GIC_CHECK_LAUNCH("gemm gumbelmax");
  return GIC_OK;
}

int gemm(const GemmDesc& d0, hipStream_t stream) {
  GemmDesc d = d0;
#ifdef GIC_STAMPS
  { const char* e = getenv("GIC_GEMM_DBG"); if (e) d.dbg = atoi(e); }
#endif
  static const bool log = getenv("GIC_GEMM_LOG") != nullptr;      // one line per product on stderr (tools: which shapes a step issues, and their routes)
  const bool probe = route_only();
  if (probe) route_line()[0] = 0;
  GIC_CHECK_ARG(d.A && d.B && d.C, "gemm: null operand");
  GIC_CHECK_ARG(d.M >= 0 && d.N >= 0 && d.K >= 0, "gemm: negative dim");
  if (d.M == 0 || d.N == 0) return GIC_OK;
  if (d.epi == EPI_HIGHWAY) GIC_CHECK_ARG(d.X, "gemm: highway epilogue needs X");      // Hpre may be null (forward only)
  const int sz = dtype_size(d.in_dtype);
  const int ve = 16 / sz;
  bool vec = plain_vec(d);
  if (d.conv) {
    // a 16-B chunk holds `ve` consecutive k = channels of one tap, or (pre-padded input, pad == 0) whole adjacent taps of one row
    const bool chunk_ok = (d.cCin % ve == 0) || (d.cPad == 0 && ve % d.cCin == 0 && (d.cKW * d.cCin) % ve == 0);
    GIC_CHECK_ARG(chunk_ok && d.K == d.cKH * d.cKW * d.cCin && d.K % ve == 0, "gemm: conv needs Cin %% %d == 0 (or a pre-padded NHWC4 stem) and K = KH*KW*Cin", ve);
    GIC_CHECK_ARG(d.epi != EPI_BNSTATS || d.stats, "gemm: EPI_BNSTATS needs a stats buffer");
    vec = aligned16(d.A) && aligned16(d.B) && (d.ldb % ve == 0);
  }
  // (plain_vec: k-contiguous operands: K must be a whole number of 16-B chunks (callers zero-pad K).  m/n-contiguous
  // operands: a tail chunk reads into the row's padding (ld % ve == 0 >= M) and only feeds rows that are
  // never stored, so no condition on M / N.)
  Plan p;
  for (int after = F_NONE;; after = p.family) {
    const int rc = select(d, vec, after, p);
    if (log || probe) {
      if (rc == GIC_OK) write_route(p);
      else snprintf(route_line(), kRouteLen, "unsupported");
      if (log && !d.conv)
        fprintf(stderr, "[gemm] M=%d N=%d K=%d a_kc=%d b_kc=%d in=%d out=%d epi=%d acc=%d -> %s\n", d.M, d.N, d.K, d.a_kc, d.b_kc, d.in_dtype, d.out_dtype,
                d.epi, d.accumulate, route_line());
    }
    if (rc != GIC_OK || probe) return rc;
    if (launch(p, stream)) break;
  }
  GIC_CHECK_LAUNCH(kFamily[p.family]);
  return GIC_OK;
}

}  // namespace gic
#ifdef GIC_STAMPS
extern "C" int gic_debug_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(gic::g_stamp), sizeof(unsigned long long) * 32);
}
#endif
