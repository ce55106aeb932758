// Shallow-K 1x1 convolutions of the ResNet trunk (torchvision conv1x1 of the bottleneck blocks, reference src/generator.py:12-14)
// as a STREAMING kernel: K = 64 or 128 input channels, a large row count, bf16, BatchNorm column sums, optional BatchNorm + ReLU of
// the input on load.
//
// With K this shallow a 128x128 output tile is 0.1 us of MFMA work behind 64-96 KB of traffic: the layer is bound by HBM
// (16 us for the widest one at 8 TB/s), and tile8 runs it at a third of that -- one workgroup per tile, each a serial chain
// (coefficient table, DMA round trip, BatchNorm rewrite, MFMAs, C tile through LDS, column sums, atomics, stores) with two workgroups
// per CU to overlap (measured with tools/conv_stamps.py: 7.5 us per workgroup, 3 of them epilogue, 1.5 prologue).  Here a
// workgroup is persistent: it keeps its 128 (or 64) output channels' weights in LDS, walks row tiles with a stride of the grid,
// streams their A tiles through an LDS-DMA ring two or three tiles ahead, accumulates the BatchNorm column sums in registers
// across all its tiles (one atomic per column and workgroup at the end) and pays the prologue once.
#include <stdlib.h>

#include "conv1x1_stream.h"
#include "bn_fold.h"
#include "conv_device.h"
#include "gemm_device.h"

namespace gic {
namespace {

// LDS image of conv1x1_stream_kernel<BN, KT, ABN, STATS>: [ring of ns A tiles of a_bytes (ns - 1 in flight) | weights: KT x BN rows x 128 B |
// unless STATS: one C tile (128 rows of sc bytes), two with KT == 1 | column sums [4 row waves][BN][2] f32 | ABN: coefficient table [64 KT][2] f32]
struct StreamLds { int ns, a_bytes, sc, c_bytes, w0, c0, st0, coef0, bytes; };
constexpr StreamLds stream_lds(int BN, int KT, bool ABN, bool STATS) {
  const int ns = KT == 1 ? 4 : 2, a_bytes = KT * 128 * 128, sc = BN * 2 + 16, c_bytes = 128 * sc;
  const int w0 = ns * a_bytes, c0 = w0 + KT * BN * 128, st0 = c0 + (STATS ? 0 : (KT == 1 ? 2 : 1) * c_bytes), coef0 = st0 + 4 * BN * 2 * 4;
  return {ns, a_bytes, sc, c_bytes, w0, c0, st0, coef0, coef0 + (ABN ? 64 * KT * 8 : 0)};
}

// everything the kernel reads from its arguments, compact (one batch of scalar loads at the top)
// BN output channels per workgroup; KT = K / 64; ABN: BatchNorm + ReLU of the input on load; STATS: the column sums ONLY (the first pass of
// conv_b2b.hip's pair: no C tile in LDS, no stores -- which leaves room for 256 output channels per workgroup, so that a row tile is
// fetched and normalised once for all of them)
template <int BN, int KT, bool ABN, bool STATS = false>
__global__ __launch_bounds__(512) void conv1x1_stream_kernel(const StreamDesc d) {
  constexpr int BM = 128, NT = 512, K = 64 * KT;
  constexpr StreamLds LY = stream_lds(BN, KT, ABN, STATS);
  constexpr int NS = LY.ns;                                             // ring stages of A tiles (NS - 1 tiles in flight)
  constexpr int TM = 2, TN = BN / 32;
  constexpr int CA = KT * 2;                                            // 16-byte pieces of an A tile per thread (128 rows x 128 B per K tile)
  constexpr int CW = KT * BN / 64;                                      // ... of the weight tile
  constexpr int CS = BM * BN * 2 / 16 / NT;                             // 16-byte stores of a C tile per thread
  constexpr int A_BYTES = LY.a_bytes, SC = LY.sc, C_BYTES = LY.c_bytes, W0 = LY.w0, C0 = LY.c0, ST0 = LY.st0, COEF0 = LY.coef0;
  constexpr bool DBUF = KT == 1;                                        // two C tiles: one barrier per row tile, the stores of a tile run under the next tile's MFMAs
  static_assert(lds_ok({A_BYTES, C_BYTES, W0, C0, ST0, COEF0}, LY.bytes), "LDS layout");
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int M = d.M, N = d.N;
  // workgroup -> (output-channel tile, first row tile): the channel tiles of one row-tile sequence are neighbours on one XCD and walk
  // their row tiles in step, so each A tile leaves HBM once (share_a; the weights, <= 128 KB, sit in every L2 anyway)
  const int bid = d.share_a ? xcd_run(blockIdx.x, gridDim.x) : blockIdx.x;
  const int tile_n = bid % d.tiles_n;
  const int grp = bid / d.tiles_n;
  const int bn0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)d.A, 0, (int)d.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)d.B, 0, (int)d.b_bytes, 0x00020000);
  const int wbase = (tid & ~63) * 16;
  // piece i of a tile: K tile i / 2 (A) , rows (tid >> 3) + 64 (i & 1), physical slot tid & 7 = logical 16-byte chunk ^ ((row >> 1) & 7)
  const int kc = swz_dma_chunk(tid) * 8;                                // this thread's 8 channels inside every 64-channel K tile
  auto issue_a = [&](const int tile, const int st) {
    const int bm0 = tile * BM;
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int row = bm0 + (tid >> 3) + 64 * (i & 1);
      const unsigned voff = (tile < d.tiles_m && row < M) ? (unsigned)(row * d.lda + (i >> 1) * 64 + kc) * 2u : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_ptr)(smem + st * A_BYTES + i * (NT * 16) + wbase), 16, (int)voff, 0, 0, GIC_TRUNK_NT);
    }
  };
  // ---- prologue: the weights of this workgroup's output channels (resident), the first NS - 1 row tiles
  constexpr int WR = BN / 64;                                           // 64-row groups of the weight tile
#pragma unroll
  for (int i = 0; i < CW; ++i) {
    const int n = bn0 + (tid >> 3) + 64 * (i % WR);
    const unsigned voff = n < N ? (unsigned)(n * d.ldb + (i / WR) * 64 + kc) * 2u : OOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_ptr)(smem + W0 + i * (NT * 16) + wbase), 16, (int)voff, 0, 0, 0);
  }
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) issue_a(grp + s * d.groups, s);

  // ---- A-side BatchNorm + ReLU: this thread's pieces always hold the same 8 channels of each K tile -> coefficients in registers
  float scl[KT][8], sft[KT][8];
  if constexpr (ABN) {
    float* coef = (float*)(smem + COEF0);
    for (int c = tid; c < K; c += NT) {                                  // (bn_fold.h's bn_scale_shift, in place: through the call this kernel's registers are allocated differently)
      const float gam = d.in_gamma[c], bet = d.in_beta[c];
      float s1, s2;
      fold_replicas(d.in_stats, d.in_nrep, K, c, s1, s2);
      const float mean = s1 * d.in_inv_count;
      const float var = fmaxf(s2 * d.in_inv_count - mean * mean, 0.f);
      const float sc = gam * rsqrtf(var + kBnEps);
      coef[2 * c] = sc;
      coef[2 * c + 1] = bet - mean * sc;
    }
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) bn_unpack8(coef + 2 * (kt * 64 + kc), scl[kt], sft[kt]);
  }

  float st_s[TN], st_q[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) st_s[j] = st_q[j] = 0.f;
  bf16_t* __restrict__ C = (bf16_t*)d.C;
  unsigned char* sC = smem + C0;

  // ---- row tiles grp, grp + groups, ...: ring stage of the j-th = j % NS
  constexpr int CPR = BN / 8;                                            // 16-byte chunks per C tile row
  auto store_tile = [&](const int bm0, const unsigned char* buf) {
    if constexpr (STATS) return;                                         // the statistics-only pass writes (and stages) nothing
#pragma unroll
    for (int i = 0; i < CS; ++i) {
      const int c = tid + NT * i;
      const int ml = c / CPR, cc = c % CPR;
      const int m = bm0 + ml, n = bn0 + cc * 8;
      const u32x4 v = *(const u32x4*)(buf + ml * SC + cc * 16);
      if (m < M && n < N) *(u32x4*)(C + (long)m * d.ldc + n) = v;      // (a wave skips a store only in its last, partial row tile)
    }
  };
  int st = 0, jj = 0, prev_bm0 = 0;
  for (int tile = grp; tile < d.tiles_m; tile += d.groups) {
    const int bm0 = tile * BM;
    // A tile j has landed once all but the DMAs and stores issued after it are done.  Per iteration a thread issues the DMA of the tile
    // NS - 1 ahead (CA pieces), then the stores of a C tile (CS; double-buffered C: of the PREVIOUS tile, so iteration 0 has none).
    if (STATS) {               // no stores in the queue: only the DMAs issued behind tile j may be outstanding
      if constexpr (DBUF) wait_vm<2 * CA>(); else wait_vm<0>();
    } else if constexpr (DBUF) {      // NS = 4: behind tile j came 2 tiles' DMAs and the stores of iterations max(1, j - 3) .. j - 1
      if (jj <= 1) wait_vm<2 * CA>();
      else if (jj == 2) wait_vm<2 * CA + CS>();
      else if (jj == 3) wait_vm<2 * CA + 2 * CS>();
      else wait_vm<2 * CA + 3 * CS>();
    } else {                   // NS = 2: tile j was issued in iteration j - 1 ahead of that iteration's stores
      if (jj == 0) wait_vm<0>(); else wait_vm<CS>();
    }
    if constexpr (ABN) {
      // rows past M were zero-filled and must stay zero (they feed rows that are never stored; keeps the sums exact)
#pragma unroll
      for (int i = 0; i < CA; ++i) {
        if (bm0 + (tid >> 3) + 64 * (i & 1) >= M) continue;
        bf16x8* p = (bf16x8*)(smem + st * A_BYTES + (tid + NT * i) * 16);
        bf16x8 v = *p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (bf16_t)fmaxf((float)v[e] * scl[i >> 1][e] + sft[i >> 1][e], 0.f);   // (bn_relu8, in place: as above)
        *p = v;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // A tile published; the previous C tile is complete; every wave is done with ring stage st - 1
    // the tile NS - 1 ahead goes into the stage that the previous tile occupied
    issue_a(tile + (NS - 1) * d.groups, st == 0 ? NS - 1 : st - 1);
    unsigned char* sCj = sC + (DBUF ? (jj & 1) * C_BYTES : 0);
    if constexpr (DBUF && !STATS) {
      if (jj > 0) store_tile(prev_bm0, sC + ((jj - 1) & 1) * C_BYTES);   // runs under this tile's MFMAs
    }
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const unsigned char* sA = smem + st * A_BYTES;
    const unsigned char* sW = smem + W0;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 fa[TM], fb[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          const int row = wr * 32 + t * 16 + lr;
          fa[t] = *(const bf16x8*)(sA + kt * (BM * 128) + row * 128 + swz_chunk(row, ks * 4 + lg));
        }
#pragma unroll
        for (int t = 0; t < TN; ++t) {
          const int row = wc * (BN / 2) + t * 16 + lr;
          fb[t] = *(const bf16x8*)(sW + kt * (BN * 128) + row * 128 + swz_chunk(row, ks * 4 + lg));
        }
        mfma_block(acc, fa, fb);
      }
    }
    // C tile -> LDS, column sums into the registers that live across tiles
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nl = wc * (BN / 2) + j * 16 + lr;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ml = wr * 32 + i * 16 + lg * 4 + r;
          const float v = acc[i][j][r];
          if constexpr (!STATS) *(bf16_t*)(sCj + ml * SC + nl * 2) = (bf16_t)v;
          if (bm0 + ml < M) { st_s[j] += v; st_q[j] += v * v; }
        }
      }
    }
    if constexpr (!DBUF && !STATS) {
      __syncthreads();
      store_tile(bm0, sCj);
    }
    prev_bm0 = bm0;
    ++jj;
    st = st == NS - 1 ? 0 : st + 1;
  }
  if constexpr (DBUF && !STATS) {
    __syncthreads();
    if (jj > 0) store_tile(prev_bm0, sC + ((jj - 1) & 1) * C_BYTES);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- BatchNorm column sums of all this workgroup's tiles: fold the 4 row groups of a wave, then the 4 row waves, one atomic per column
  float* sStat = (float*)(smem + ST0);                                   // [4 row waves][BN][2]
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    float s = st_s[j], q = st_q[j];
    s += __shfl_xor(s, 16, 64); q += __shfl_xor(q, 16, 64);
    s += __shfl_xor(s, 32, 64); q += __shfl_xor(q, 32, 64);
    if (lg == 0) {
      const int nl = wc * (BN / 2) + j * 16 + lr;
      sStat[(wr * BN + nl) * 2] = s;
      sStat[(wr * BN + nl) * 2 + 1] = q;
    }
  }
  __syncthreads();
  if (tid < BN && bn0 + tid < N) {
    float s0 = 0.f, q0 = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { s0 += sStat[(r * BN + tid) * 2]; q0 += sStat[(r * BN + tid) * 2 + 1]; }
    float* stp = d.stats + (long)(blockIdx.x % d.stats_nrep) * 2 * N;
    atomicAdd(&stp[bn0 + tid], s0);
    atomicAdd(&stp[N + bn0 + tid], q0);
  }
}

template <int BN, int KT, bool ABN, bool STATS = false>
bool launch_stream(const StreamPlan& p, hipStream_t stream) {
  static LdsGrant granted;
  if (!grant_lds(conv1x1_stream_kernel<BN, KT, ABN, STATS>, p.lds, granted)) return false;
  hipLaunchKernelGGL((conv1x1_stream_kernel<BN, KT, ABN, STATS>), dim3(p.grid), dim3(512), p.lds, stream, p.d);
  return true;
}

}  // namespace

bool select_conv1x1_stream(const GemmDesc& d, StreamPlan& p) {
  static const bool off = getenv("GIC_NO_CONV1X1_STREAM") != nullptr;
  static const int min_tiles = [] { const char* e = getenv("GIC_STREAM_MIN_TILES"); return e ? atoi(e) : 1024; }();
  if (off || d.res) return false;
  if (d.cKH != 1 || d.cKW != 1 || d.cStride != 1 || d.cPad != 0) return false;
  if ((d.K != 64 && d.K != 128) || d.cCin != d.K || d.lda != d.K) return false;
  if (d.N % 8 || d.ldc % 8 || d.ldb % 8 || (long)d.M * d.ldc * 2 >= (1l << 40)) return false;
  StreamDesc& sd = p.d;
  if (!conv_base(d, (long)d.M * d.K, (long)(d.N - 1) * d.ldb + d.K, sd)) return false;
  static const bool bn64 = getenv("GIC_STREAM_BN64") != nullptr;
  static const int wg_per_cu = [] { const char* e = getenv("GIC_STREAM_WG_PER_CU"); return e ? atoi(e) : 1; }();
  p.abn = d.in_stats != nullptr;
  // the statistics-only pass (input normalised on load, output channels a multiple of 256): 256 channels per workgroup
  p.stats = d.stats_only && p.abn && d.N % 256 == 0;
  if (d.stats_only && !p.stats) return false;
  p.BN = p.stats ? 256 : (d.N >= 128 && !bn64 ? 128 : 64);
  p.KT = d.K / 64;
  sd.tiles_m = cdiv(d.M, 128);
  sd.tiles_n = cdiv(d.N, p.BN);
  // streaming pays where a workgroup walks several row tiles; small grids stay with tile8 (counted in 128-wide tiles for both forms)
  if ((long)sd.tiles_m * (p.stats ? d.N / 128 : sd.tiles_n) < min_tiles) return false;
  int groups = 256 * wg_per_cu / sd.tiles_n;           // one persistent workgroup per CU (the ring + the C tile fill most of its LDS)
  if (groups < 1) groups = 1;
  if (groups > sd.tiles_m) groups = sd.tiles_m;
  sd.groups = groups;
  sd.share_a = xcd_share_a(2l * d.M * d.K, 2l * d.N * d.K, sd.tiles_n);
  sd.stats_only = d.stats_only;
  p.grid = (unsigned)(sd.groups * sd.tiles_n);
  p.lds = (size_t)stream_lds(p.BN, p.KT, p.abn, p.stats).bytes;
  return true;
}

bool launch_conv1x1_stream(const StreamPlan& p, hipStream_t stream) {
  const bool kt1 = p.KT == 1;
  if (p.stats) return kt1 ? launch_stream<256, 1, true, true>(p, stream) : launch_stream<256, 2, true, true>(p, stream);
  switch (p.BN + p.abn) {
    case 128 + 1: return kt1 ? launch_stream<128, 1, true>(p, stream) : launch_stream<128, 2, true>(p, stream);
    case 64 + 1: return kt1 ? launch_stream<64, 1, true>(p, stream) : launch_stream<64, 2, true>(p, stream);
    case 128 + 0: return kt1 ? launch_stream<128, 1, false>(p, stream) : launch_stream<128, 2, false>(p, stream);
    case 64 + 0: return kt1 ? launch_stream<64, 1, false>(p, stream) : launch_stream<64, 2, false>(p, stream);
  }
  return false;
}

}  // namespace gic
