// 1x1 convolutions with K = 256 input channels and many output channels (conv3 of the 14x14 bottlenecks of the ResNet trunk: 256 ->
// 1024, reference src/generator.py:12-14) with the A PANEL of a 128-row tile RESIDENT in LDS: loaded (and, with BatchNorm + ReLU on
// load, normalised) once, then multiplied with the output-channel tiles of the workgroup's group one after the other while their
// weight tiles stream through a two-stage LDS-DMA ring.
//
// tile8 runs such a layer as 784 independent 128x128 tiles: every one of the eight tiles of a row block fetches the same 64 KB of
// A, rewrites it with the same coefficients and pays its own coefficient table, DMA round trips (ring-less: one per K tile) and
// drain (measured 27 us per launch against an HBM floor of 4 us, 11.5 us per workgroup of which 7 us are the serial K tiles).
#include <stdlib.h>

#include "conv1x1_panel.h"
#include "bn_fold.h"
#include "conv_device.h"
#include "gemm_device.h"

namespace gic {
namespace {

// LDS image of conv1x1_panel_kernel<KT, ABN>: [A panel: KT x 128 rows x 128 B | two weight stages of w_bytes | C tile: 128 rows of sc bytes |
// column sums [8 waves][32][2] f32 | ABN: coefficient table [64 KT][2] f32]
struct PanelLds { int w_bytes, sc, w0, c0, st0, coef0, bytes; };
constexpr PanelLds panel_lds(int KT, bool ABN) {
  const int w_bytes = KT * 64 * 128, sc = 64 * 2 + 16, w0 = KT * 128 * 128, c0 = w0 + 2 * w_bytes, st0 = c0 + 128 * sc, coef0 = st0 + 8 * 32 * 2 * 4;
  return {w_bytes, sc, w0, c0, st0, coef0, coef0 + (ABN ? 64 * KT * 8 : 0)};
}

// everything the kernel reads from its arguments, compact (one batch of scalar loads at the top)
// KT = K / 64 (4); ABN: BatchNorm + ReLU of the input on load.  8 waves as 4 (M) x 2 (N): a wave owns 32 x 32 of a 128 x 64 output tile.
template <int KT, bool ABN>
__global__ __launch_bounds__(512) void conv1x1_panel_kernel(const PanelDesc d) {
  constexpr int BM = 128, BN = 64, NT = 512, K = 64 * KT;
  constexpr int TM = 2, TN = 2;
  constexpr int CA = KT * 2;                                            // 16-byte pieces of the A panel per thread
  constexpr int CW = KT;                                                // ... of a weight tile (64 rows x 128 B per K tile)
  constexpr int CS = BM * BN * 2 / 16 / NT;                             // 16-byte stores of a C tile per thread (2)
  constexpr PanelLds LY = panel_lds(KT, ABN);
  constexpr int W_BYTES = LY.w_bytes, SC = LY.sc, W0 = LY.w0, C0 = LY.c0, ST0 = LY.st0, COEF0 = LY.coef0;
  static_assert(lds_ok({W0, C0, ST0, COEF0}, LY.bytes), "LDS layout");
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int M = d.M, N = d.N;
  // workgroup -> (row tile, group of output-channel tiles): the groups of one row tile are neighbours on one XCD (they share the A panel
  // in its L2: xcd_run)
  const int bid = d.share_a ? xcd_run(blockIdx.x, gridDim.x) : blockIdx.x;
  const int grp = bid % d.groups, tile_m = bid / d.groups;
  const int bm0 = tile_m * BM;
  const int nt0 = grp * d.per_group;
  const int nt1 = min(nt0 + d.per_group, d.tiles_n);

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A, 0, (int)d.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)d.B, 0, (int)d.b_bytes, 0x00020000);
  const int wbase = (tid & ~63) * 16;
  const int kc = swz_dma_chunk(tid) * 8;                                // this thread's 8 channels inside every 64-channel K tile

  // ---- prologue: the A panel (piece i: K tile i / 2, rows (tid >> 3) + 64 (i & 1)), the first weight tile
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int row = bm0 + (tid >> 3) + 64 * (i & 1);
    const unsigned voff = row < M ? (unsigned)(row * d.lda + (i >> 1) * 64 + kc) * 2u : OOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_ptr)(smem + i * (NT * 16) + wbase), 16, (int)voff, 0, 0, GIC_TRUNK_NT);
  }
  auto issue_w = [&](const int nt, const int st) {                      // weight tile nt: piece i = K tile i, rows tid >> 3
    const int n = nt * BN + (tid >> 3);
#pragma unroll
    for (int i = 0; i < CW; ++i) {
      const unsigned voff = (nt < nt1 && n < N) ? (unsigned)(n * d.ldb + i * 64 + kc) * 2u : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_ptr)(smem + W0 + st * W_BYTES + i * (NT * 16) + wbase), 16, (int)voff, 0, 0, 0);
    }
  };
  issue_w(nt0, 0);

  if constexpr (ABN) {
    float* coef = (float*)(smem + COEF0);
    for (int c = tid; c < K; c += NT) bn_scale_shift(d.in_stats, d.in_nrep, K, c, d.in_inv_count, d.in_gamma, d.in_beta, coef[2 * c], coef[2 * c + 1]);
    __syncthreads();
    wait_vm<CW>();                                                       // the panel has landed (the weight tile may be in flight)
    // a thread's pieces of K tile kt all hold channels kt*64 + kc .. + 7; rows past M were zero-filled and stay zero
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      if (bm0 + (tid >> 3) + 64 * (i & 1) >= M) continue;
      float scl[8], sft[8];
      bn_unpack8(coef + 2 * ((i >> 1) * 64 + kc), scl, sft);
      bf16x8* p = (bf16x8*)(smem + (tid + NT * i) * 16);
      *p = bn_relu8(*p, scl, sft);
    }
  }

  bf16_t* __restrict__ C = (bf16_t*)d.C;
  unsigned char* sC = smem + C0;
  float* sStat = (float*)(smem + ST0);                                   // [8 waves][BN/2][2]
  int st = 0;
  for (int nt = nt0; nt < nt1; ++nt) {
    const int bn0 = nt * BN;
    // weight tile nt: behind it came only the previous tile's stores (wave 0: + its two atomics; waiting for all but CS is the
    // stricter count there).  The first tile waits for everything (panel included).
    // A partial row tile skips stores in some waves (their counts differ): it waits for everything.
    if (nt == nt0 || bm0 + BM > M) wait_vm<0>(); else wait_vm<CS>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // weights (and, first tile, the normalised panel) published; the other stage and the C tile are free
    issue_w(nt + 1, st ^ 1);
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const unsigned char* sW = smem + W0 + st * W_BYTES;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 fa[TM], fb[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          const int row = wr * 32 + t * 16 + lr;
          fa[t] = *(const bf16x8*)(smem + kt * (BM * 128) + row * 128 + swz_chunk(row, ks * 4 + lg));
        }
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const int row = wc * (BN / 2) + t * 16 + lr;
          fb[t] = *(const bf16x8*)(sW + kt * (BN * 128) + row * 128 + swz_chunk(row, ks * 4 + lg));
        }
        mfma_block(acc, fa, fb);
      }
    }
    // C tile through LDS, BatchNorm column sums folded across the workgroup (as tile8)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nl = wc * (BN / 2) + j * 16 + lr;
      float st_s = 0.f, st_q = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ml = wr * 32 + i * 16 + lg * 4 + r;
          const float v = acc[i][j][r];
          *(bf16_t*)(sC + ml * SC + nl * 2) = (bf16_t)v;
          if (bm0 + ml < M) { st_s += v; st_q += v * v; }
        }
      }
      st_s += __shfl_xor(st_s, 16, 64); st_q += __shfl_xor(st_q, 16, 64);
      st_s += __shfl_xor(st_s, 32, 64); st_q += __shfl_xor(st_q, 32, 64);
      if (lg == 0) { sStat[(w * (BN / 2) + j * 16 + lr) * 2] = st_s; sStat[(w * (BN / 2) + j * 16 + lr) * 2 + 1] = st_q; }
    }
    __syncthreads();
    if (tid < BN) {                                                      // column tid (all of wave 0): waves (wr = 0..3, wc)
      const int cwc = tid / (BN / 2), cl = tid % (BN / 2), n = bn0 + tid;
      float s0 = 0.f, q0 = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s0 += sStat[((r * 2 + cwc) * (BN / 2) + cl) * 2];
        q0 += sStat[((r * 2 + cwc) * (BN / 2) + cl) * 2 + 1];
      }
      if (n < N) {
        float* stp = d.stats + (long)(blockIdx.x % d.stats_nrep) * 2 * N;
        atomicAdd(&stp[n], s0);
        atomicAdd(&stp[N + n], q0);
      }
    }
    constexpr int CPR = BN / 8;
#pragma unroll
    for (int i = 0; i < CS; ++i) {
      const int c = tid + NT * i;
      const int ml = c / CPR, cc = c % CPR;
      const int m = bm0 + ml, n = bn0 + cc * 8;
      const u32x4 v = *(const u32x4*)(sC + ml * SC + cc * 16);
      if (m < M && n < N) *(u32x4*)(C + (long)m * d.ldc + n) = v;
    }
    st ^= 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // (the zero-fill DMA of the tile past the group)
}

template <int KT, bool ABN>
bool launch_panel(const PanelPlan& p, hipStream_t stream) {
  static LdsGrant granted;
  if (!grant_lds(conv1x1_panel_kernel<KT, ABN>, p.lds, granted)) return false;
  hipLaunchKernelGGL((conv1x1_panel_kernel<KT, ABN>), dim3(p.grid), dim3(512), p.lds, stream, p.d);
  return true;
}

}  // namespace

bool select_conv1x1_panel(const GemmDesc& d, PanelPlan& p) {
  static const bool off = getenv("GIC_NO_CONV1X1_PANEL") != nullptr;
  if (off || d.res) return false;
  if (d.cKH != 1 || d.cKW != 1 || d.cStride != 1 || d.cPad != 0) return false;
  if (d.K != 256 || d.cCin != d.K || d.lda != d.K || d.N < 512 || d.N % 64 || d.ldc % 8 || d.ldb % 8) return false;      // the panel pays where it serves many tiles
  PanelDesc& pd = p.d;
  if (!conv_base(d, (long)d.M * d.K, (long)(d.N - 1) * d.ldb + d.K, pd)) return false;
  pd.tiles_m = cdiv(d.M, 128);
  pd.tiles_n = d.N / 64;
  // about one workgroup per CU: split the output-channel tiles of a row tile over as many groups as that leaves room for
  int groups = 256 / pd.tiles_m;
  if (groups < 1) groups = 1;
  if (groups > pd.tiles_n) groups = pd.tiles_n;
  pd.per_group = cdiv(pd.tiles_n, groups);
  pd.groups = cdiv(pd.tiles_n, pd.per_group);
  pd.share_a = xcd_share_a(2l * d.M * d.K, 2l * d.N * d.K, pd.groups);
  p.KT = 4; p.abn = d.in_stats != nullptr;
  p.grid = (unsigned)(pd.tiles_m * pd.groups);
  p.lds = (size_t)panel_lds(p.KT, p.abn).bytes;
  return true;
}

bool launch_conv1x1_panel(const PanelPlan& p, hipStream_t stream) {
  return p.abn ? launch_panel<4, true>(p, stream) : launch_panel<4, false>(p, stream);
}

}  // namespace gic
